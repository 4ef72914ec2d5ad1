"""Shared by tests/test_wave_linalg.py (host build of tests/probe/wave_probe.hip) and tests/test_gpu_wave_linalg.py
(device build): the probe loader, the case tables and the assertions against tests/wave_linalg_reference.py.

Conventions.  A Jacobi result is (X, Y, G, W): X the N input rows of length M, Y = G X the rotated rows (row i =
sigma_i u_i), G the accumulated rotations (N x N), W the row norms, all four in descending order of W.  eps is
DBL_EPSILON = 2^-52 and ||X|| the spectral norm from mpmath.  Why the bounds hold: every pair is left at or
below 10 eps non-orthogonal and at most 30 sweeps of (1 + O(eps)) rotations follow, so 64 N eps has room to spare."""
import ctypes as C
import os
import subprocess

import mpmath as mp
import numpy as np

import wave_linalg_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE_DIR = os.path.join(HERE, "probe")
DEVICE_LIB = os.path.join(PROBE_DIR, "libwave_probe.so")
HOST_LIB = os.path.join(HERE, "sim", "_build", "libwave_probe_sim.so")
EPS = ref.EPS

# entry -> (doubles in, doubles out) per case; wave_probe.hip refuses anything else
SIZES = dict(svd3=(9, 21), svd4=(16, 36), svd3_ls=(9, 63), jrr12_hyp=(144, 312), jrr12_ref=(144, 312), jrr6=(36, 84),
             jrr6x9=(54, 66), jrr10=(100, 220), eig8=(64, 72), solve6x3=(24, 9), solve6x4=(30, 12), solve6x5=(36, 15),
             solve3x3=(18, 9), nearest_rot=(9, 9), qr6x4=(30, 4), rodrigues_fwd=(3, 36), rodrigues_inv=(9, 3),
             decompose_essential=(9, 21), roots10=(11, 11), five_point=(20, 114))


class Probe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        for name in SIZES:
            fn = getattr(self.lib, "probe_" + name)
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
            fn.restype = C.c_int

    def raw(self, name, inp, out, n, nin, nout):
        return getattr(self.lib, "probe_" + name)(inp.ctypes.data_as(C.c_void_p) if inp is not None else None,
                                                  out.ctypes.data_as(C.c_void_p) if out is not None else None, n, nin, nout)

    def run(self, name, cases):
        """cases: n arrays (any shape, nin doubles each) -> [n, nout] doubles."""
        nin, nout = SIZES[name]
        inp = np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.float64).ravel() for c in cases]))
        assert inp.shape[1] == nin, (name, inp.shape)
        out = np.full((len(inp), nout), np.nan)
        rc = self.raw(name, inp, out, len(inp), nin, nout)
        assert rc == 0, "probe_%s returned %d" % (name, rc)
        return out


def load_probe(kind):
    """kind 'host' or 'device'.  make rebuilds the library when it is older than its sources."""
    subprocess.check_call(["make", "-C", PROBE_DIR, "-s"] + (["host"] if kind == "host" else []))
    if kind != "host":
        # as the package's load_library: torch bundles its own libamdhip64, and when both end up in one process
        # torch's must be loaded first, or a later torch.cuda call of another test finds no GPU
        import torch  # noqa: F401
    return Probe(HOST_LIB if kind == "host" else DEVICE_LIB)


# ---------------------------------------------------------------------------------------------------------------------
# case tables
def _orth(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _with_spectrum(rng, n, m, s):
    """N x M matrix with the given singular values (up to rounding) behind random rotations."""
    k = min(n, m)
    core = np.zeros((n, m))
    core[np.arange(k), np.arange(k)] = np.asarray(s, dtype=np.float64)[:k]
    return _orth(rng, n) @ core @ _orth(rng, m)


def row_cases(n, m, seed):
    """[(label, X)]: N rows of length M for the Jacobi family."""
    rng = np.random.RandomState(seed)
    k = min(n, m)
    out = [("random%d" % i, rng.standard_normal((n, m))) for i in range(4)]
    out.append(("pixels", rng.uniform(-1e4, 1e4, (n, m))))
    one_one_zero = np.r_[1.0, 1.0, np.zeros(k - 2)]
    out += [("ones_spectrum", _with_spectrum(rng, n, m, np.ones(k))),
            ("one_one_zero", _with_spectrum(rng, n, m, one_one_zero)),
            ("graded_1e-16", _with_spectrum(rng, n, m, np.logspace(0, -16, k))),
            ("graded_1_1e-8_1e-16", _with_spectrum(rng, n, m, np.r_[1.0, 1e-8, np.full(k - 2, 1e-16)])),
            ("graded_1e-8", _with_spectrum(rng, n, m, np.logspace(0, -8, k))),
            ("repeated_pairs", _with_spectrum(rng, n, m, np.repeat(np.arange(k, 0, -2.0), 2)[:k]))]
    z = rng.standard_normal((n, m))
    z[n - 1] = 0
    out.append(("zero_row", z))
    z = rng.uniform(-3, 3, (n, m))
    z[0] = 0
    out.append(("zero_first_row", z))
    z = rng.standard_normal((n, m))
    z[1] = z[0]
    out.append(("equal_rows", z))
    out += [("rank1", np.outer(rng.standard_normal(n), rng.standard_normal(m))),
            ("zero", np.zeros((n, m)))]
    d = np.zeros((n, m))
    d[np.arange(k), np.arange(k)] = np.arange(k, 0, -1.0)
    out.append(("diag_descending", d))
    out.append(("diag_ascending", np.flipud(d).copy()))
    t = np.zeros((n, m))
    t[np.arange(k), np.arange(k)] = np.where(np.arange(k) % 2 == 0, 2.0, 1.0)
    out.append(("diag_ties", t))
    p = np.zeros((n, m))
    p[np.arange(k), rng.permutation(m)[:k]] = 1.0
    out.append(("permutation", p))
    # many sweeps: nearly parallel rows (all ones + 1e-9 noise), Hilbert rows, rows differing in the last place
    out.append(("near_parallel", np.ones((n, m)) + 1e-9 * rng.standard_normal((n, m))))
    out.append(("hilbert", 1.0 / (np.arange(n)[:, None] + np.arange(m)[None, :] + 1.0)))
    out.append(("ones_plus_ulp", np.ones((n, m)) + EPS * rng.randint(0, 4, (n, m))))
    out += [("scale_1e60", 1e60 * rng.standard_normal((n, m))), ("scale_1e-60", 1e-60 * rng.standard_normal((n, m)))]
    return out


def gram_cases(n, seed):
    """Symmetric positive semi-definite n x n inputs: column-scaled Gram matrices M^T M as EPnP forms them (five points
    give 10 rows, hence rank <= 10 of 12), lower ranks, well-conditioned, graded and clustered spectra."""
    rng = np.random.RandomState(seed)
    scale = np.where(np.arange(n) % 3 == 2, 300.0, 500.0) * rng.uniform(0.1, 1.0, n)   # (a fu, a fv, a (uc - u)) columns
    out = []
    for rows in (10, 4, n + 4):
        if rows >= n and rows != n + 4:
            continue
        m = rng.standard_normal((rows, n)) * scale
        out.append(("gram_rank%d_scaled" % min(rows, n), m.T @ m))
    m = rng.standard_normal((min(10, n - 2), n))
    out.append(("gram_unscaled", m.T @ m))
    q = _orth(rng, n)
    for label, s in (("sym_graded_1e-12", np.logspace(0, -12, n)), ("sym_clustered", np.r_[np.full(n // 2, 3.0), np.full(n - n // 2, 1.0)]),
                     ("sym_identityish", np.ones(n))):
        a = (q * s) @ q.T
        out.append((label, (a + a.T) / 2))
    out.append(("sym_diag_ties", np.diag(np.where(np.arange(n) % 2 == 0, 2.0, 1.0))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Jacobi family: unpacking and assertions
def unpack_rows(out, n, m, with_g=True, with_perm=False):
    """One probe output row -> (Y, G or None, W) in descending order (jacobi_rr's perm applied)."""
    y = out[:n * m].reshape(n, m)
    o = n * m
    g = None
    if with_g:
        g = out[o:o + n * n].reshape(n, n)
        o += n * n
    w = out[o:o + n]
    perm = None
    if with_perm:
        perm = out[o + n:o + 2 * n].astype(int)
        assert sorted(perm.tolist()) == list(range(n)), "perm is no permutation: %r" % (out[o + n:o + 2 * n],)
        y, w = y[perm], w[perm]
        g = g[perm] if g is not None else None
    return y, g, w, perm


def jacobi_errors(x, y, g, w):
    """The figures the Jacobi bounds are about, each already divided by its bound's scale: reconstruction
    |X - G^T Y|_max / ||X||, orthogonality of G, orthogonality of the normalised non-null rows of Y, singular values
    |W - sigma|_max / sigma_max, and | |Y_i| - W_i | / sigma_max.  A row is non-null when its norm exceeds the accuracy
    64 N eps sigma_max the singular values themselves are held to."""
    n, m = x.shape
    assert np.isfinite(y).all() and np.isfinite(w).all() and (g is None or np.isfinite(g).all()), "non-finite output"
    sig = ref.singular_values(x)
    smax = sig[0] if sig[0] > 0 else mp.mpf(1)
    Y = ref.M(y)
    res = {}
    if g is not None:
        G = ref.M(g)
        res["reconstruction"] = ref.max_abs(ref.M(x) - G.T * Y) / float(smax)
        res["orth_G"] = ref.max_abs(G * G.T - mp.eye(n))
    k = min(n, m)
    full = [sig[i] if i < k else mp.mpf(0) for i in range(n)]
    res["sigma"] = float(max(abs(mp.mpf(float(w[i])) - full[i]) for i in range(n)) / smax)
    norms = [mp.sqrt(mp.fsum(Y[i, j] ** 2 for j in range(m))) for i in range(n)]
    res["row_norm"] = float(max(abs(norms[i] - mp.mpf(float(w[i]))) for i in range(n)) / smax)
    live = [i for i in range(n) if norms[i] > 64 * n * EPS * smax]
    worst = mp.mpf(0)
    for a in live:
        for b in live:
            if a < b:
                worst = max(worst, abs(mp.fsum(Y[a, j] * Y[b, j] for j in range(m)) / (norms[a] * norms[b])))
    res["orth_rows"] = float(worst)
    res["rank"] = len(live)
    return res


def assert_jacobi(label, x, y, g, w, worst=None):
    n, m = x.shape
    e = jacobi_errors(x, y, g, w)
    if worst is not None:
        for key in ("reconstruction", "orth_G", "orth_rows", "sigma", "row_norm"):
            if key in e:
                worst[key] = max(worst.get(key, 0.0), e[key])
    # Largest values measured over all tables, host build and MI355X alike (the two agree bit for bit): reconstruction
    # 9.8e-16 (12 x 12; bound 1.7e-13), G G^T - I 2.8e-15, rotated rows 2.2e-15, singular values 8.4e-16 sigma_max
    # (bound 1.7e-13 each at N = 12, 4.3e-14 at N = 3, where 4.2e-16, 7.4e-16, 1.5e-15 and 1.7e-16 were measured).
    if g is not None:
        assert e["reconstruction"] <= 64 * max(m, n) * EPS, "%s: reconstruction %.3g" % (label, e["reconstruction"])
        assert e["orth_G"] <= 64 * n * EPS, "%s: G G^T - I %.3g" % (label, e["orth_G"])
    assert e["orth_rows"] <= 64 * n * EPS, "%s: rotated rows not orthogonal %.3g" % (label, e["orth_rows"])
    assert e["sigma"] <= 64 * n * EPS, "%s: singular values off by %.3g sigma_max" % (label, e["sigma"])
    assert e["row_norm"] <= 64 * n * EPS, "%s: W is not the norm of its row (%.3g)" % (label, e["row_norm"])
    assert (np.diff(w) <= 0).all(), "%s: W not descending: %r" % (label, w)
    return e


def assert_ties_keep_input_order(label, x, y, g, w):
    """Inputs whose rows are orthogonal already (diagonal, permutation): no rotation happens, so Y is X with its rows
    ordered by norm, equal norms in input order, and G is that permutation matrix exactly."""
    norms = np.sqrt((x * x).sum(1))
    order = np.argsort(-norms, kind="stable")
    assert np.array_equal(y, x[order]), "%s: rows not in stable descending order" % label
    assert np.array_equal(w, norms[order]), label
    if g is not None:
        assert np.array_equal(g, np.eye(len(x))[order]), "%s: G is not the stable permutation" % label


def projector_gap_check(label, a, g, tol_scale):
    """Symmetric a: the eigenvectors of each cluster of mpmath's eigenvalues (neighbours closer than 1e-6 lambda_max
    share a cluster) span the same subspace as the matching rows of G; Davis-Kahan with the backward error
    tol_scale * ||a|| gives |P - P_ref|_max <= tol_scale * ||a|| / gap.  Returns the worst ratio to that bound."""
    n = len(a)
    lam, vec = ref.eigsy(a)
    top = max(abs(lam[0]), abs(lam[-1]))
    if top == 0:
        return 0.0
    clusters, start = [], 0
    for i in range(1, n + 1):
        if i == n or lam[i - 1] - lam[i] > mp.mpf("1e-6") * top:
            clusters.append((start, i))
            start = i
    G = ref.M(g)
    worst = 0.0
    for lo, hi in clusters:
        gaps = ([lam[lo - 1] - lam[lo]] if lo > 0 else []) + ([lam[hi - 1] - lam[hi]] if hi < n else [])
        if not gaps:
            continue
        gap = min(gaps)
        P = mp.zeros(n)
        Pr = mp.zeros(n)
        for i in range(lo, hi):
            P += G[i, :].T * G[i, :]
            Pr += vec[i] * vec[i].T
        bound = tol_scale * float(top / gap)
        err = ref.max_abs(P - Pr)
        assert err <= bound, "%s: eigenspace %d..%d off by %.3g (bound %.3g)" % (label, lo, hi - 1, err, bound)
        worst = max(worst, err / bound)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# rotations
AXIS = np.array([1.0, -2.0, 3.0]) / np.sqrt(14.0)      # not aligned with any coordinate axis
SMALL = 1e-5 * np.sqrt(2.0)
ANGLES = [0.0, 1e-12, 1e-8, np.nextafter(SMALL, 0), SMALL, np.nextafter(SMALL, 1), 1e-4, 1.0, np.pi - 1e-4, np.pi - 1e-8, np.pi]


def rotation_matrix(theta):
    """The rotation by theta about AXIS, rounded to double from the mpmath closed form."""
    return ref.as_float(ref.rodrigues([mp.mpf(float(a)) * mp.mpf(float(theta)) for a in AXIS]))


def ulp_distance(a, b):
    """Largest distance in units of the last place between two double arrays (NaN against NaN and equal values 0)."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    both_nan = np.isnan(a) & np.isnan(b)
    if (np.isnan(a) != np.isnan(b)).any():
        return np.inf
    a, b = a[~both_nan], b[~both_nan]
    if not len(a):
        return 0.0
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
    d[a == b] = 0
    return float(d.max())


# ---------------------------------------------------------------------------------------------------------------------
# polynomials
def poly_from_roots(real, pairs=()):
    """Double coefficients (leading first, 11 of them) of the product over the real roots and the complex pairs
    (re, im), formed in mpmath and rounded once."""
    c = [mp.mpf(1)]
    for r in real:
        c = _polymul(c, [mp.mpf(1), -mp.mpf(float(r))])
    for re, im in pairs:
        re, im = mp.mpf(float(re)), mp.mpf(float(im))
        c = _polymul(c, [mp.mpf(1), -2 * re, re * re + im * im])
    c = [float(x) for x in c]
    return np.array([0.0] * (11 - len(c)) + c)


def _polymul(a, b):
    out = [mp.mpf(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] += x * y
    return out


def span_poly(decades, rng=None):
    """Ten real roots of both signs whose magnitudes spread evenly (in the exponent) over `decades` decades, centred
    on 1; with rng the exponents are drawn instead of spread."""
    e = np.linspace(-decades / 2.0, decades / 2.0, 10) if rng is None else np.sort(rng.uniform(-decades / 2.0, decades / 2.0, 10))
    sign = np.array([1, 1, -1, 1, -1, 1, 1, -1, 1, -1.0])
    return poly_from_roots(sign * 10.0 ** e)


SPANS = (2, 4, 6, 8, 10, 12)
TWELVE_DECADES = np.poly([1e-6, 1e-3, .1, 1, 10, 1e3, 1e6, -1, -100, -1e4])


def poly_cases(seed=5):
    """[(label, c11)] the regular table: the finder is expected to return every real root of each."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(30):        # random real coefficients: 0 to 10 real roots, mostly 2 to 4
        out.append(("random_coeffs%d" % i, rng.standard_normal(11)))
    for i in range(25):        # ten real roots within one decade of 1
        out.append(("ten_real%d" % i, poly_from_roots(rng.uniform(-3, 3, 10))))
    for i in range(25):        # mixed: k real roots and (10 - k) / 2 complex pairs
        k = 2 * rng.randint(0, 5)
        out.append(("mixed%d" % i, poly_from_roots(rng.uniform(-5, 5, k), [(rng.uniform(-2, 2), rng.uniform(0.1, 2)) for _ in range((10 - k) // 2)])))
    for lead in (1, 2, 5, 9):  # leading zeros: degree 10 - lead
        c = poly_from_roots(rng.uniform(-3, 3, 10 - lead))
        assert (c[:lead] == 0).all()
        out.append(("leading_zeros%d" % lead, c))
    out.append(("no_real_root", poly_from_roots([], [(rng.uniform(-2, 2), rng.uniform(0.5, 2)) for _ in range(5)])))
    out.append(("no_real_root_x10_plus_1", np.r_[1.0, np.zeros(9), 1.0]))
    for i in range(6):         # two roots 1e-6 apart among well separated ones
        r = rng.uniform(-3, 3)
        others = [x for x in np.linspace(-4, 4, 9) if abs(x - r) > 0.3][:8]
        out.append(("close_1e-6_%d" % i, poly_from_roots([r, r + 1e-6] + others)))
    for i in range(6):         # a complex pair 1e-8 from the real axis
        out.append(("pair_1e-8_%d" % i, poly_from_roots(rng.uniform(-3, 3, 8), [(rng.uniform(-3, 3), 1e-8)])))
    return out


def double_root_cases():
    """Exact double roots: integer roots, so the coefficients are exact and the double root is one of the polynomial
    as the finder sees it."""
    return [("double_at_1", poly_from_roots([1, 1, -2, 3, -4, 5, -6, 7, -8, 9])),
            ("double_at_0", poly_from_roots([0, 0, -2, 3, -4, 5, -6, 7, -8, 9])),
            ("two_doubles", poly_from_roots([2, 2, -3, -3, 1, 4, -5, 6, -7, 8])),
            ("double_and_pairs", poly_from_roots([1, 1, -2, 3], [(0, 1), (1, 2), (-1, 1)]))]


def root_check(c, out):
    """One polynomial against mpmath: dict(count, ref_count, worst, problems, decidable).

    A reference real root z is held to tol = 4 ulp(z) max(1, kappa_z).  Where tol reaches half the distance from z to
    the nearest other root (real or complex) the tolerance itself can no longer tell the two apart -- a perturbation
    of the coefficients within the same 4 ulp merges them or moves them off the axis -- so neither "within tol" nor
    the number of real roots is a property of the double coefficients there.  Such roots, and complex pairs whose
    imaginary part is within their own tol, are `loose`: the finder may return them or not.  Every other real root
    must be returned exactly once within tol, and every returned root must be one of those or lie at a loose root.
    `decidable` says there was no loose root, and then the counts are equal whenever `problems` is empty.  `worst` is
    the largest |root - ref| / tol over the matched roots."""
    real, cond, sep, cpx = ref.all_roots(c)
    n = int(out[0])
    assert 0 <= n <= 10, out
    got = [mp.mpf(float(r)) for r in out[1:1 + n]]
    assert all(np.isfinite(out[1:1 + n])) and all(a <= b for a, b in zip(got, got[1:])), "roots not finite and ascending: %r" % (out,)
    tol = [4 * float(np.spacing(abs(float(z)))) * max(1.0, k) for z, k in zip(real, cond)]
    used, problems, worst, loose = set(), [], 0.0, []
    for z, t, s in zip(real, tol, sep):
        if not t < s / 2:
            loose.append((z, max(t, s)))
            continue
        near = [i for i, r in enumerate(got) if i not in used and abs(r - z) <= t]
        if len(near) != 1:
            problems.append("root %.17g (kappa tol %.3g) returned %d times" % (float(z), t, len(near)))
            continue
        used.add(near[0])
        worst = max(worst, float(abs(got[near[0]] - z)) / t)
    for w, k in cpx:
        t = 4 * float(np.spacing(abs(float(w.real)))) * max(1.0, k)
        if abs(w.imag) <= t:
            loose.append((w.real, t))
    for i, r in enumerate(got):
        if i not in used and not any(abs(r - z) <= reach for z, reach in loose):
            problems.append("returned %.17g is no root" % float(r))
    return dict(count=n, ref_count=len(real), worst=worst, problems=problems, decidable=not loose)


def matched_roots(c, out):
    """How many of the reference's real roots the finder returned (each within 1e-6 relative), and the reference."""
    want, _ = ref.real_roots(c)
    got = out[1:1 + int(out[0])]
    hit = [any(abs(mp.mpf(float(r)) - z) <= mp.mpf("1e-6") * abs(z) for r in got) for z in want]
    return hit, want


# ---------------------------------------------------------------------------------------------------------------------
# five-point polynomials from synthetic key-frame scenes
def five_point_samples(synth, seed, motion, n_samples, pix_noise):
    """Normalised 5-point samples (q1 [S,5,2], q2 [S,5,2]) of one two-view scene.  The scene points are
    synth.keyframe_problem(seed)'s; `motion` picks the second view: 'keyframe' keeps the problem's own pose and pixels,
    'forward' moves 0.25 along the optical axis with a 1e-3 sideways component and no rotation, 'short' keeps the
    rotation-free sideways motion but a baseline of a hundredth of the mean depth."""
    kf = synth.keyframe_problem(n=200, seed=seed, pix_noise=pix_noise, outlier_frac=0.0)
    K = kf["K"]
    f = (K["fx"] + K["fy"]) / 2
    rng = np.random.RandomState(1000 + seed)
    if motion == "keyframe":
        k1, k2 = kf["kp_ref"].astype(np.float64), kf["kp_cur"].astype(np.float64)
    else:
        p = kf["p_ref"]
        t = np.array([1e-3, 0.0, 0.25]) if motion == "forward" else np.array([0.01 * p[:, 2].mean(), 0.0, 0.0])
        q = p - t

        def pix(x):
            uv = np.stack([K["fx"] * x[:, 0] / x[:, 2] + K["cx"], K["fy"] * x[:, 1] / x[:, 2] + K["cy"]], 1)
            return (uv + rng.normal(0, pix_noise, uv.shape) if pix_noise else uv).astype(np.float32).astype(np.float64)
        k1, k2 = pix(p), pix(q)
    c = np.array([K["cx"], K["cy"]])
    q1, q2 = (k1 - c) / f, (k2 - c) / f
    idx = np.stack([rng.choice(len(q1), 5, replace=False) for _ in range(n_samples)])
    return q1[idx], q2[idx]


# ---------------------------------------------------------------------------------------------------------------------
# The checks.  Each takes a Probe (host or device build) and returns the figures it measured, so the test modules can
# print them; CHECKS lists them for parametrisation.
ROW_ENTRIES = {          # entry -> (N, M, has G, has perm, copies of the result, symmetric cases too)
    "svd4": (4, 4, True, False, 1, False),
    "svd3_ls": (3, 3, True, False, 3, False),
    "jrr12_hyp": (12, 12, True, True, 1, True),
    "jrr12_ref": (12, 12, True, True, 1, True),
    "jrr6": (6, 6, True, True, 1, True),
    "jrr6x9": (6, 9, False, True, 1, False),
    "jrr10": (10, 10, True, True, 1, True),
}
ORDER_PINNED = ("diag_descending", "diag_ascending", "diag_ties", "permutation", "sym_diag_ties", "zero")


def row_inputs(entry):
    n, m, _, _, _, sym = ROW_ENTRIES[entry]
    seed = 100 + 10 * n + m
    return row_cases(n, m, seed) + (gram_cases(n, seed + 1) if sym else [])


def check_rows(P, entry):
    n, m, has_g, has_perm, copies, _ = ROW_ENTRIES[entry]
    cases = row_inputs(entry)
    out = P.run(entry, [x for _, x in cases])
    worst = {}
    for (label, x), o in zip(cases, out):
        per = len(o) // copies
        for k in range(1, copies):      # every wave's copy of the result is the same
            assert np.array_equal(o[:per], o[k * per:(k + 1) * per], equal_nan=True), "%s %s: wave %d differs" % (entry, label, k)
        y, g, w, _ = unpack_rows(o[:per], n, m, has_g, has_perm)
        assert_jacobi("%s %s" % (entry, label), x, y, g, w, worst)
        if label in ORDER_PINNED:
            assert_ties_keep_input_order("%s %s" % (entry, label), x, y, g, w)
        if g is not None and (label.startswith("gram") or label.startswith("sym")):
            worst["eigenspace/bound"] = max(worst.get("eigenspace/bound", 0.0),
                                            projector_gap_check("%s %s" % (entry, label), x, g, 64 * n * EPS))
    return worst


def svd3_inputs():
    return row_cases(3, 3, 133)


def check_svd3(P):
    """svd3(A) with A = X^T, so that the rows the Jacobi works on are the table's rows."""
    cases = svd3_inputs()
    out = P.run("svd3", [x.T for _, x in cases])
    worst, completed = {}, 0
    for (label, x), o in zip(cases, out):
        U, w, V = o[:9].reshape(3, 3), o[9:12], o[12:].reshape(3, 3)
        y, g = (U * w).T, V.T
        assert_jacobi("svd3 " + label, x, y, g, w, worst)
        sig = ref.singular_values(x)
        live = [i for i in range(3) if sig[i] > 64 * 3 * EPS * sig[0]]
        Ul = ref.M(U[:, live]) if live else None
        if live:
            e = ref.max_abs(Ul.T * Ul - mp.eye(len(live)))
            worst["orth_U"] = max(worst.get("orth_U", 0.0), e)
            assert e <= 64 * 3 * EPS, "svd3 %s: U^T U - I %.3g on the non-null columns" % (label, e)
        if not w[2] > np.finfo(np.float64).tiny and len(live) == 2:
            # the completion: a third singular value of exactly zero gets u2 = u0 x u1, a full orthogonal U
            completed += 1
            Um = ref.M(U)
            e = ref.max_abs(Um.T * Um - mp.eye(3))
            assert e <= 64 * 3 * EPS, "svd3 %s: completed U not orthogonal (%.3g)" % (label, e)
            assert abs(mp.det(Um) - 1) <= 64 * 3 * EPS, "svd3 %s: u2 is not u0 x u1" % label
    assert completed >= 2, "the table no longer reaches svd3's completion of a zero singular value"
    return worst


def eig8_inputs():
    return gram_cases(8, 88)


def check_eig8(P):
    cases = eig8_inputs()
    out = P.run("eig8", [a for _, a in cases])
    worst = {}
    for (label, a), o in zip(cases, out):
        w, E = o[:8], o[8:].reshape(8, 8)
        assert np.isfinite(o).all(), label
        lam, _ = ref.eigsy(a)
        top = float(lam[0])
        Em = ref.M(E)
        fig = dict(reconstruction=ref.max_abs(ref.M(a) - Em.T * mp.diag([mp.mpf(float(x)) for x in w]) * Em) / top,
                   orth_E=ref.max_abs(Em * Em.T - mp.eye(8)),
                   eigenvalues=float(max(abs(mp.mpf(float(w[i])) - lam[i]) for i in range(8))) / top)
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 64 * 8 * EPS, "eig8 %s: %s %.3g" % (label, k, v)
        assert (np.diff(w) <= 0).all(), label
        worst["eigenspace/bound"] = max(worst.get("eigenspace/bound", 0.0), projector_gap_check("eig8 " + label, a, E, 64 * 8 * EPS))
        if label == "sym_diag_ties":
            assert np.array_equal(E, np.eye(8)[np.argsort(-np.diag(a), kind="stable")]), "eig8: ties not in input order"
    return worst


# ---- solves
def solve_inputs(rows, cols, seed):
    """[(label, A, b)].  The graded systems take b in the range of A: the kappa^2 term of least-squares perturbation
    theory, which the bound does not carry, is proportional to the residual."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(4):
        out.append(("random%d" % i, rng.standard_normal((rows, cols)), rng.standard_normal(rows)))
    out.append(("epnp_like", rng.standard_normal((rows, cols)) * rng.uniform(1, 100, cols), rng.uniform(0, 50, rows)))
    for kappa in (1e4, 1e8, 1e12):
        a = _with_spectrum(rng, rows, cols, np.logspace(0, -np.log10(kappa), cols))
        out.append(("graded_%g" % kappa, a, a @ rng.standard_normal(cols)))
    a = rng.standard_normal((rows, cols))
    a[:, cols - 1] = 0
    out.append(("zero_column", a, rng.standard_normal(rows)))
    a = rng.standard_normal((rows, cols))
    a[:, 1] = a[:, 0]
    out.append(("equal_columns", a, a @ rng.standard_normal(cols)))
    a = _with_spectrum(rng, rows, cols, np.r_[np.ones(cols - 1), 0.0])
    out.append(("rank_deficient_rotated", a, a @ rng.standard_normal(cols)))
    out.append(("zero", np.zeros((rows, cols)), rng.standard_normal(rows)))
    return out


def _solve_error(label, a, b, x, n):
    """|x - x_ref|_2 relative to the bound 64 N eps kappa |x_ref| (kappa over the singular values the documented rule
    keeps); a system that keeps none must give exactly zero."""
    xr, sig, kept = ref.lstsq(a, b)
    assert np.isfinite(x).all(), label
    if kept == 0:
        assert not x.any(), "%s: nothing survives the truncation, x must be 0" % label
        return 0.0
    kappa = sig[0] / sig[kept - 1]
    diff = ref.M(x.reshape(xr.rows, xr.cols)) - xr
    err = mp.sqrt(mp.fsum(v * v for v in diff))
    bound = 64 * n * EPS * kappa * mp.sqrt(mp.fsum(v * v for v in xr))
    assert err <= bound, "%s: |x - x_ref| %.3g > %.3g (kappa %.3g, kept %d of %d)" % (label, float(err), float(bound), float(kappa), kept, len(sig))
    return float(err / bound) if bound > 0 else 0.0


def check_solve6(P, nc):
    entry = "solve6x%d" % nc
    cases = solve_inputs(6, nc, 60 + nc)
    out = P.run(entry, [np.r_[a.ravel(), b] for _, a, b in cases])
    worst = 0.0
    for (label, a, b), o in zip(cases, out):
        for k in (1, 2):
            assert np.array_equal(o[:nc], o[k * nc:(k + 1) * nc]), "%s %s: wave %d differs" % (entry, label, k)
        worst = max(worst, _solve_error("%s %s" % (entry, label), a, b, o[:nc], nc))
    return {"error/bound": worst}


def solve3_inputs():
    rng = np.random.RandomState(33)
    out = []
    for label, a, _ in solve_inputs(3, 3, 34):
        out.append((label + "_eye", a, np.eye(3)))      # the product inverts the control-point basis
        out.append((label, a, rng.standard_normal((3, 3)) if "random" in label else a @ rng.standard_normal((3, 3))))
    return out


def check_solve3(P):
    cases = solve3_inputs()
    out = P.run("solve3x3", [np.r_[a.ravel(), b.ravel()] for _, a, b in cases])
    worst = 0.0
    for (label, a, b), o in zip(cases, out):
        if label.endswith("_eye") and not label.startswith("random") and not label.startswith("epnp"):
            continue    # pinv of an ill-conditioned A against I has a residual: outside the bound's theory (see solve_inputs)
        worst = max(worst, _solve_error("solve3x3 " + label, a, b, o, 3))
    return {"error/bound": worst}


def qr_inputs():
    cases = [c for c in solve_inputs(6, 4, 64) if c[0].startswith(("random", "epnp", "graded", "zero"))]
    rng = np.random.RandomState(65)
    a = rng.standard_normal((6, 4))
    a[:, 0] = 0
    cases.append(("zero_first_column", a, rng.standard_normal(6)))
    return cases


def check_qr(P):
    """Full rank: the least-squares solution.  A column that is zero from the diagonal down makes qr_solve_6x4 declare
    the system singular, and its singular outcome is x = 0."""
    cases = qr_inputs()
    out = P.run("qr6x4", [np.r_[a.ravel(), b] for _, a, b in cases])
    worst = 0.0
    for (label, a, b), o in zip(cases, out):
        if label.startswith("zero"):
            assert np.array_equal(o, np.zeros(4)), "qr6x4 %s: singular outcome is x = 0, got %r" % (label, o)
        else:
            worst = max(worst, _solve_error("qr6x4 " + label, a, b, o, 4))
    return {"error/bound": worst}


def nearest_rot_inputs():
    rng = np.random.RandomState(77)
    out = []
    for i in range(4):
        r = _orth(rng, 3)
        r *= np.sign(np.linalg.det(r))
        out.append(("noisy_rotation%d" % i, r + 1e-3 * rng.standard_normal((3, 3))))
        out.append(("scaled_rotation%d" % i, 10.0 ** rng.randint(-3, 4) * r))
    for i in range(4):
        a = rng.standard_normal((3, 3))
        out.append(("random_det+%d" % i, a * np.sign(np.linalg.det(a))))
    out.append(("identity", np.eye(3)))
    out.append(("near_singular", _with_spectrum(rng, 3, 3, [1.0, 0.5, 1e-6])))
    out.append(("random_det-", -out[-3][1]))
    return [(l, a if l == "random_det-" or np.linalg.det(a) > 0 else a * np.array([1, 1, -1.0])) for l, a in out]


def check_nearest_rot(P):
    cases = nearest_rot_inputs()
    out = P.run("nearest_rot", [a for _, a in cases])
    worst = {}
    for (label, a), o in zip(cases, out):
        R = ref.M(o.reshape(3, 3))
        Q, sig = ref.polar_rotation(a)
        gap = (sig[1] + sig[2]) / sig[0]        # the polar factor moves by 2 |dA| / (sigma_2 + sigma_3)
        fig = dict(orth=ref.max_abs(R.T * R - mp.eye(3)), polar=ref.max_abs(R - Q) * float(gap))
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 64 * 3 * EPS, "nearest_rot %s: %s %.3g" % (label, k, v)
        if label != "random_det-":
            assert np.linalg.det(a) > 0 and mp.det(R) >= 0, "nearest_rot %s: det R < 0 for det A > 0" % label
    return worst


# ---- rotations
def _axis_mp():
    return [mp.mpf(float(a)) for a in AXIS]


INV_ZERO_BELOW = 1e-5    # rodrigues_inv: sin(theta) < 1e-5 with cos > 0 gives the zero vector, with cos < 0 the near-pi formula
INV_ANGLES = ANGLES + [0.99e-5, 1.01e-5]


def check_rodrigues_fwd(P):
    rs = [AXIS * th for th in ANGLES]
    out = P.run("rodrigues_fwd", rs)
    worst = {}
    for th, r, o in zip(ANGLES, rs, out):
        Rm, J = ref.rodrigues(r), ref.rodrigues_jacobian(r)
        eR = float(max(abs(mp.mpf(float(o[k])) - Rm[k // 3, k % 3]) for k in range(9)))
        eJ = float(max(abs(mp.mpf(float(o[9 + 9 * i + k])) - J[i][k]) for i in range(3) for k in range(9)))
        bound = 16 * EPS * max(1.0, th)
        worst["R/bound"] = max(worst.get("R/bound", 0.0), eR / bound)
        worst["J/bound"] = max(worst.get("J/bound", 0.0), eJ / bound)
        assert eR <= bound, "rodrigues_fwd theta %.17g: R off by %.3g (bound %.3g)" % (th, eR, bound)
        assert eJ <= bound, "rodrigues_fwd theta %.17g: dR/dr off by %.3g (bound %.3g)" % (th, eJ, bound)
    return worst


def check_rodrigues_inv(P):
    """The normal branch against the true rotation vector and through rodrigues_fwd again; the two special branches
    pinned.  Tolerance of the normal branch: theta = acos(c) with c = (tr R - 1) / 2 taken from a matrix that
    nearest_rotation_uvt holds to 64 * 3 eps per entry, so |dc| <= 1.5 * 64 * 3 eps and |dtheta| <= |dc| / sin(theta);
    together with the 16 eps max(1, theta) of the forward map: 16 eps max(1, theta) + 288 eps / sin(theta)."""
    Rs = [rotation_matrix(th) for th in INV_ANGLES]
    out = P.run("rodrigues_inv", Rs)
    normal = [i for i, th in enumerate(INV_ANGLES) if np.sin(th) >= 1.005e-5]
    back = P.run("rodrigues_fwd", [out[i] for i in normal])
    worst = {}
    for i, (th, o) in enumerate(zip(INV_ANGLES, out)):
        true = AXIS * th
        err = np.abs(o - true).max()
        if np.sin(th) < 0.995e-5 and np.cos(th) > 0:
            # OpenCV's small-angle branch: the zero vector, whatever the angle -- off by the angle itself, up to 1e-5
            assert np.array_equal(o, np.zeros(3)), "rodrigues_inv theta %.3g: the small-angle branch returns 0, got %r" % (th, o)
            worst["small-angle branch error"] = max(worst.get("small-angle branch error", 0.0), err)
            assert err <= INV_ZERO_BELOW
        elif np.sin(th) < 0.995e-5:
            # OpenCV's near-pi branch: axis from the diagonal, angle from acos(c) near c = -1, which resolves the
            # angle only to sqrt(2 |dc|) with |dc| <= 288 eps as above
            worst["near-pi branch error"] = max(worst.get("near-pi branch error", 0.0), err)
            assert err <= np.sqrt(2 * 288 * EPS) * np.pi, "rodrigues_inv theta pi - %.3g: off by %.3g" % (np.pi - th, err)
        else:
            tol = 16 * EPS * max(1.0, th) + 288 * EPS / np.sin(th)
            worst["normal branch/bound"] = max(worst.get("normal branch/bound", 0.0), err / tol)
            assert err <= tol, "rodrigues_inv theta %.17g: off by %.3g (bound %.3g)" % (th, err, tol)
            Rb = back[normal.index(i)][:9].reshape(3, 3)
            rt = np.abs(Rb - Rs[i]).max()
            worst["round trip/bound"] = max(worst.get("round trip/bound", 0.0), rt / tol)
            assert rt <= tol, "round trip theta %.17g: off by %.3g (bound %.3g)" % (th, rt, tol)
    return worst


def essential_inputs():
    rng = np.random.RandomState(91)
    out = []
    for i in range(8):
        r = _orth(rng, 3)
        r *= np.sign(np.linalg.det(r))
        t = rng.standard_normal(3)
        if i == 0:
            t = np.array([0.0, 0.0, 1.0])     # forward motion
        if i == 1:
            t = np.array([1.0, 0.0, 0.0])
            r = np.eye(3)                       # pure sideways translation
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        e = tx @ r
        for label, s in (("unit", 1 / np.linalg.norm(e)), ("negated", -1.0), ("by_e22", 1 / e[2, 2] if abs(e[2, 2]) > 1e-3 else 3.0)):
            out.append(("E%d_%s" % (i, label), e * s))
    return out


def check_decompose_essential(P):
    cases = essential_inputs()
    out = P.run("decompose_essential", [e for _, e in cases])
    worst = {}
    bound = 64 * 3 * EPS
    for (label, e), o in zip(cases, out):
        R1, R2, t = ref.M(o[:9].reshape(3, 3)), ref.M(o[9:18].reshape(3, 3)), ref.M(o[18:])
        tx = mp.matrix([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        E = ref.M(e)
        En = E / mp.sqrt(mp.fsum(v * v for v in E))
        fig = {"det": float(max(abs(mp.det(R1) - 1), abs(mp.det(R2) - 1))),
               "orth": max(ref.max_abs(R1.T * R1 - mp.eye(3)), ref.max_abs(R2.T * R2 - mp.eye(3))),
               "|t|": float(abs(mp.sqrt(mp.fsum(v * v for v in t)) - 1))}
        for name, R in (("[t]x R1", R1), ("[t]x R2", R2)):
            F = tx * R
            Fn = F / mp.sqrt(mp.fsum(v * v for v in F))
            fig[name] = min(ref.max_abs(Fn - En), ref.max_abs(Fn + En))
        assert ref.max_abs(R1 - R2) > 0.1, "%s: R1 and R2 are the same rotation" % label
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= bound, "decompose_essential %s: %s off by %.3g" % (label, k, v)
    return worst


# ---- roots
AGREED_SPAN = 6          # decades: the largest span of the table at which the finder returns every root (see below)


def span_inputs():
    rng = np.random.RandomState(3)
    out = []
    for d in SPANS:
        out.append((d, "spread", span_poly(d)))
        for i in range(5):
            out.append((d, "drawn%d" % i, span_poly(d, rng)))
    return out


def roots_inputs():
    return poly_cases() + [("root_at_an_interval_end", poly_from_roots([0, 1, 2, 3, -1, -2, 0.5, 4, -3, 5])),
                           ("root_at_zero_then_pairs", poly_from_roots([0, 1.5], [(1, 1), (-1, 2), (0.5, 0.5), (2, 1)]))]


ROOT_GROUPS = ("random_coeffs", "ten_real", "mixed", "structured", "span")


def check_roots_table(P, group):
    """One group of the regular table: random_coeffs, ten_real, mixed, structured (everything else of roots_inputs) or
    span (the spans up to AGREED_SPAN decades)."""
    if group == "span":
        cases = [("span%d_%s" % (d, l), c) for d, l, c in span_inputs() if d <= AGREED_SPAN]
    elif group == "structured":
        cases = [(l, c) for l, c in roots_inputs() if not l.startswith(ROOT_GROUPS[:3])]
    else:
        cases = [(l, c) for l, c in roots_inputs() if l.startswith(group)]
    assert cases
    out = P.run("roots10", [c for _, c in cases])
    worst, undecidable, total = 0.0, 0, 0
    for (label, c), o in zip(cases, out):
        res = root_check(c, o)
        assert not res["problems"], "%s: %s (returned %d, mpmath %d)" % (label, "; ".join(res["problems"]), res["count"], res["ref_count"])
        if res["decidable"]:
            assert res["count"] == res["ref_count"], label
        else:       # only where the table asks for it: roots 1e-6 apart, complex pairs 1e-8 from the axis
            assert label.startswith(("close_1e-6", "pair_1e-8")), "%s: not decidable at 4 ulp kappa" % label
            undecidable += 1
        worst = max(worst, res["worst"])
        total += res["ref_count"]
    return {"polynomials": len(cases), "real roots": total, "worst error/tolerance": worst, "undecidable": undecidable}


def check_roots_span_limit(P):
    """Pins where real_roots_deg10 starts to lose roots: none up to AGREED_SPAN decades on the table, the first at 8
    decades (two neighbouring small roots of one polynomial), a third of all roots at 12 decades, and 8 of 10 on the
    twelve-decade polynomial TWELVE_DECADES (1e-6 and 1e-3 missing).  The Sturm remainders are not
    normalised, so their coefficients spread over hundreds of decades and the counts near the small roots go wrong.
    No root returned is ever wrong; roots go missing."""
    cases = span_inputs()
    out = P.run("roots10", [c for _, _, c in cases])
    lost = {d: 0 for d in SPANS}
    for (d, label, c), o in zip(cases, out):
        hit, want = matched_roots(c, o)
        assert len(want) == 10
        assert int(o[0]) <= 10 and int(o[0]) == sum(hit), "span %d %s: a returned value is no root" % (d, label)
        lost[d] += 10 - sum(hit)
    first = min([d for d in SPANS if lost[d]] or [None])
    assert all(lost[d] == 0 for d in SPANS if d <= AGREED_SPAN), lost
    assert first == 8, "roots now start to go missing at %r decades (were: 8): %r" % (first, lost)
    o = P.run("roots10", [TWELVE_DECADES])[0]
    hit, want = matched_roots(TWELVE_DECADES, o)
    missing = sorted(float(z) for z, h in zip(want, hit) if not h)
    assert int(o[0]) == 8 and len(missing) == 2 and abs(missing[0] - 1e-6) < 1e-12 and abs(missing[1] - 1e-3) < 1e-9, (o, missing)
    return {"roots lost per span (of 60)": lost, "first span with a loss": first, "twelve-decade polynomial": "8 of 10"}


def check_roots_double(P):
    """Exact multiple roots are outside the finder's contract (the polynomial's sign does not change there): a double
    root comes back twice, once or not at all, and where it comes back it is located only to the square root of the
    evaluation noise (2.4e-9 here), hence the 1e-6.  Pinned: every value returned is a root, and every simple root is
    returned, unless the multiple root sits at 0 -- always the first bisection point, where the whole chain vanishes
    and the counts on both sides are wrong."""
    res = {}
    for label, c in double_root_cases():
        o = P.run("roots10", [c])[0]
        want, _ = ref.real_roots(c)
        got = o[1:1 + int(o[0])]
        assert all(any(abs(mp.mpf(float(r)) - z) <= mp.mpf("1e-6") * max(1, abs(z)) for z in want) for r in got), (label, got)
        mult = [z for z in want if abs(mp.polyval([mp.mpf(float(x)) * (10 - i) for i, x in enumerate(c[:10])], z)) < mp.mpf("1e-30")]
        simple = [z for z in want if z not in mult]
        found = sum(any(abs(mp.mpf(float(r)) - z) <= mp.mpf("1e-6") * max(1, abs(z)) for r in got) for z in simple)
        res[label] = "%d of %d simple roots, %d values" % (found, len(simple), len(got))
        if label != "double_at_0":
            assert found == len(simple), "%s: %s" % (label, res[label])
    return res


# ---- scales
def check_scales(P):
    """svd3 on a well-conditioned 3 x 3 matrix times 1e150 and 1e-200: the squared row norms overflow or underflow, and
    the function has no flag for it.  Pinned: at 1e150 the result is non-finite or not an SVD, at 1e-200 every singular
    value is zero.  The callers cannot come near either: they feed normalised image coordinates (about 1), pixel
    coordinates (up to about 1e4), depths and their products of degree at most four, so entries stay within 1e-60 ..
    1e60, where the squares stay within 1e-120 .. 1e120 and the usual bounds hold."""
    rng = np.random.RandomState(150)
    a = rng.standard_normal((3, 3)) + 2 * np.eye(3)
    res = {}
    for s in (1e60, 1e-60, 1e30, 1e-30):
        o = P.run("svd3", [(a * s).T])[0]
        U, w, V = o[:9].reshape(3, 3), o[9:12], o[12:].reshape(3, 3)
        e = assert_jacobi("svd3 scale %g" % s, a * s, (U * w).T, V.T, w)
        res["scale %g" % s] = "reconstruction %.2g" % e["reconstruction"]
    o = P.run("svd3", [(a * 1e150).T])[0]
    U, w = o[:9].reshape(3, 3), o[9:12]
    sig = np.array([float(x) for x in ref.singular_values(a)]) * 1e150
    broken = (not np.isfinite(o).all()) or np.abs(U.T @ U - np.eye(3)).max() > 1e-3 or np.abs(w / sig - 1).max() > 1e-3
    assert broken, "svd3 at scale 1e150 now gives a finite SVD: the range it handles has grown, update this test"
    res["scale 1e150"] = "finite %s, W / sigma %r" % (np.isfinite(o).all(), (w / sig).tolist())
    o = P.run("svd3", [(a * 1e-200).T])[0]
    assert np.array_equal(o[9:12], np.zeros(3)), "svd3 at scale 1e-200 no longer returns W = 0: %r" % (o[9:12],)
    res["scale 1e-200"] = "W = 0"
    return res


# ---- five-point polynomials
FIVE_POINT_SCENES = [(motion, noise) for motion in ("keyframe", "forward", "short") for noise in (0.3, 0.0)]


def five_point_inputs(synth):
    cases = []
    for k, (motion, noise) in enumerate(FIVE_POINT_SCENES):
        q1, q2 = five_point_samples(synth, (3, 6, 8)[k % 3], motion, 8, noise)
        cases += [("%s noise %g #%d" % (motion, noise, i), np.r_[a.ravel(), b.ravel()]) for i, (a, b) in enumerate(zip(q1, q2))]
    return cases


def check_five_point_span(P, synth):
    """The degree-10 polynomials five_point_hypothesis really forms (read back from the Sturm chain's first row), on
    key-frame scenes including near-pure forward motion, a baseline of a hundredth of the depth and noise-free pixels:
    every real root is found, and the roots stay inside the AGREED_SPAN decades the finder handles (measured: 3.0
    decades at most on this table, 4.2 on 216 samples of the same scenes)."""
    cases = five_point_inputs(synth)
    out = P.run("five_point", [x for _, x in cases])
    spans, total, cands = [], 0, 0
    for (label, _), o in zip(cases, out):
        assert o[1] == 10, "%s: degree %r" % (label, o[1])
        c = o[2:13]
        res = root_check(c, np.r_[o[13], o[14:24]])
        assert not res["problems"], "%s: %s" % (label, "; ".join(res["problems"]))
        assert (not res["decidable"]) or res["count"] == res["ref_count"], label
        want, _ = ref.real_roots(c)
        mags = [abs(float(z)) for z in want if z != 0]
        if len(mags) >= 2:
            spans.append(np.log10(max(mags) / min(mags)))
        total += len(want)
        cands += int(o[0])
        assert int(o[0]) <= res["count"]
    assert max(spans) <= AGREED_SPAN, "five-point root spans now reach %.1f decades" % max(spans)
    return {"polynomials": len(cases), "real roots": total, "E candidates": cands, "largest span (decades)": round(max(spans), 2)}


def check_bad_arguments(P):
    """The probe refuses what it cannot run instead of launching it."""
    nin, nout = SIZES["svd3"]
    inp, out = np.zeros((1, nin)), np.zeros((1, nout))
    assert P.raw("svd3", None, out, 1, nin, nout) == -1 and P.raw("svd3", inp, None, 1, nin, nout) == -1
    assert P.raw("svd3", inp, out, 0, nin, nout) == -2 and P.raw("svd3", inp, out, 1 << 20, nin, nout) == -2
    assert P.raw("svd3", inp, out, 1, nin + 1, nout) == -3 and P.raw("svd3", inp, out, 1, nin, nout - 1) == -3
    return {}


def bit_inputs(synth):
    """entry -> list of inputs: every case of every table, for the device-against-host comparison."""
    inputs = {e: [x for _, x in row_inputs(e)] for e in ROW_ENTRIES}
    inputs["svd3"] = [x.T for _, x in svd3_inputs()]
    inputs["eig8"] = [a for _, a in eig8_inputs()]
    for nc in (3, 4, 5):
        inputs["solve6x%d" % nc] = [np.r_[a.ravel(), b] for _, a, b in solve_inputs(6, nc, 60 + nc)]
    inputs["solve3x3"] = [np.r_[a.ravel(), b.ravel()] for _, a, b in solve3_inputs()]
    inputs["qr6x4"] = [np.r_[a.ravel(), b] for _, a, b in qr_inputs()]
    inputs["nearest_rot"] = [a for _, a in nearest_rot_inputs()]
    inputs["decompose_essential"] = [e for _, e in essential_inputs()]
    inputs["roots10"] = [c for _, c in roots_inputs()] + [c for _, _, c in span_inputs()] + [c for _, c in double_root_cases()] + [TWELVE_DECADES]
    inputs["five_point"] = [x for _, x in five_point_inputs(synth)]
    inputs["rodrigues_fwd"] = [AXIS * th for th in ANGLES]
    inputs["rodrigues_inv"] = [rotation_matrix(th) for th in INV_ANGLES]
    return inputs


TRIG_ENTRIES = ("rodrigues_fwd", "rodrigues_inv")      # sin / cos / acos: compared to 4 ulp, everything else bit for bit
