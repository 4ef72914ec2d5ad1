"""High-precision references for the small linear algebra of the wave solvers (tests/test_wave_linalg.py and
tests/test_gpu_wave_linalg.py).  Everything here is mpmath at 60 digits working on the exact values of the doubles it
is given; nothing comes from the oracle, whose Jacobi is the library's own algorithm restated."""
import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 60
EPS = 2.0 ** -52          # DBL_EPSILON, "2^-53 * 2"


def M(a):
    """numpy array (1-D or 2-D) -> mp.matrix holding the same doubles exactly."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        return mp.matrix([mp.mpf(float(x)) for x in a])
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in a])


def as_float(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def max_abs(m):
    return float(max([abs(x) for x in m] + [mp.mpf(0)]))


def _key(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.shape, a.tobytes()


@functools.lru_cache(maxsize=None)
def _svd_cached(shape, raw):
    a = np.frombuffer(raw, dtype=np.float64).reshape(shape)
    if not a.any():
        return None, [mp.mpf(0)] * min(shape), None
    U, S, V = mp.svd_r(M(a), full_matrices=False, compute_uv=True)
    return U, [S[i] for i in range(len(S))], V


def svd(a):
    """(U, [sigma descending], Vt) of a, thin; the zero matrix gives (None, zeros, None).  Cached per matrix."""
    return _svd_cached(*_key(a))


def singular_values(a):
    return svd(a)[1]


@functools.lru_cache(maxsize=None)
def _eigsy_cached(shape, raw):
    a = np.frombuffer(raw, dtype=np.float64).reshape(shape)
    E, Q = mp.eigsy(M(a))
    order = sorted(range(len(E)), key=lambda i: -E[i])
    return [E[i] for i in order], [Q[:, i] for i in order]


def eigsy(a):
    """Eigenvalues (descending) and eigenvectors (columns, same order) of the symmetric matrix a."""
    return _eigsy_cached(*_key(a))


def lstsq(a, b, drop_rel=2 * EPS):
    """Minimum-norm least-squares x of a x = b from the mpmath SVD, with the rule the library documents: a singular
    value at or below drop_rel * (sum of the singular values) is dropped.  Returns (x as mp.matrix n x nb, sigmas,
    number kept)."""
    a = np.asarray(a, dtype=np.float64)
    U, S, Vt = svd(a)
    B = M(np.asarray(b, dtype=np.float64).reshape(a.shape[0], -1))
    x = mp.zeros(a.shape[1], B.cols)
    if U is None:
        return x, S, 0
    thr = mp.fsum(S) * drop_rel
    kept = 0
    for i, s in enumerate(S):
        if s <= thr:
            continue
        kept += 1
        x += Vt[i, :].T * ((U[:, i].T * B) / s)
    return x, S, kept


def polar_rotation(a):
    """U Vt of the SVD of a 3 x 3 matrix: the orthogonal polar factor."""
    U, S, Vt = svd(a)
    return U * Vt, S


def rodrigues(r):
    """Closed-form rotation matrix exp([r]x) as an mp.matrix; r: three mpf or floats."""
    r = [mp.mpf(x) for x in r]
    th = mp.sqrt(mp.fsum(x * x for x in r))
    K = mp.matrix([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    if th == 0:
        return mp.eye(3) + K
    return mp.eye(3) + (mp.sin(th) / th) * K + ((1 - mp.cos(th)) / th ** 2) * (K * K)


def rodrigues_jacobian(r):
    """dR/dr by mp.diff: J[i][k] = d R_k / d r_i, k row-major (the library's layout)."""
    r = [mp.mpf(float(x)) for x in r]
    J = [[None] * 9 for _ in range(3)]
    with mp.workdps(120):
        for i in range(3):
            for k in range(9):
                def f(x, i=i, k=k):
                    q = list(r)
                    q[i] = x
                    return rodrigues(q)[k // 3, k % 3]
                J[i][k] = mp.diff(f, r[i])
    return J


def rotation_log(R):
    """The rotation vector of an mp rotation matrix with angle well inside (0, pi)."""
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    v = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    s = mp.sqrt(mp.fsum(x * x for x in v)) / 2
    th = mp.atan2(s, c)
    return [x * th / (2 * s) for x in v]


@functools.lru_cache(maxsize=None)
def _roots_cached(raw):
    c = [mp.mpf(float(x)) for x in np.frombuffer(raw, dtype=np.float64)]
    while c and c[0] == 0:
        c = c[1:]
    if len(c) < 2:
        return (), (), (), ()
    roots = mp.polyroots(c, maxsteps=400, extraprec=600)
    tiny = mp.mpf("1e-40")
    real = sorted(z.real for z in roots if abs(z.imag) < tiny)
    distinct = []
    for z in real:      # an exact multiple root counts once, as a Sturm sequence counts it
        if not distinct or abs(z - distinct[-1]) > tiny * max(1, abs(z)):
            distinct.append(z)
    upper = [z for z in roots if z.imag >= tiny]       # one of each conjugate pair
    dc = [c[i] * (len(c) - 1 - i) for i in range(len(c) - 1)]

    def cond(z):        # relative condition number of the root with respect to the coefficients
        if z == 0:
            return 0.0      # a zero root is a zero constant term: no relative perturbation moves it
        num = mp.fsum(abs(ci) * abs(z) ** (len(c) - 1 - i) for i, ci in enumerate(c))
        den = abs(z) * abs(mp.polyval(dc, z))
        return float(num / den) if den > 0 else float("inf")

    everything = [mp.mpc(z) for z in distinct] + upper + [z.conjugate() for z in upper]
    seps = [float(min([abs(mp.mpc(z) - w) for w in everything if abs(mp.mpc(z) - w) > tiny * max(1, abs(z))] or [mp.inf]))
            for z in distinct]
    return tuple(distinct), tuple(cond(z) for z in distinct), tuple(seps), tuple((z, cond(z)) for z in upper)


def real_roots(c):
    """Distinct real roots (ascending, mpf) of the polynomial with double coefficients c (leading first) and the
    condition number of each; mp.polyroots with raised extraprec, real when |imag| < 1e-40."""
    return _roots_cached(np.ascontiguousarray(c, dtype=np.float64).tobytes())[:2]


def all_roots(c):
    """(real roots, their condition numbers, each one's distance to the nearest other root of any kind, the complex
    roots with positive imaginary part as (root, condition number))."""
    return _roots_cached(np.ascontiguousarray(c, dtype=np.float64).tobytes())
