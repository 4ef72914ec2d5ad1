"""Numpy transcription of the map-point refresh (include/mvo_hip.h: mvo_map_refresh), written from the
declared arithmetic and sharing no code with the product: the medoid descriptor of a point's observations (ORB-SLAM's
MapPoint::ComputeDistinctiveDescriptors) and the mean of their unit viewing directions (MapPoint::UpdateNormalAndDepth).  Every
f64 operation is a numpy scalar operation in the written order.  Known answers: tests/test_map_refresh_numpy.py."""
import numpy as np

from epipolar_numpy import hamming

MAX_OBS = 64


def medians(desc):
    """med[k] of the m observations of one point: element (m - 1) // 2 of row k of D (D[k][k] = 0 included) sorted ascending."""
    D = hamming(desc, desc)
    return np.sort(D, axis=1)[:, (len(D) - 1) // 2]


def medoid(desc):
    """-> (choice, med): the k with the smallest med[k], the lowest k on a tie."""
    med = medians(desc)
    return int(np.argmin(med)), med          # argmin returns the first of equal minima


def normal(pos_f32, cams):
    """The mean unit viewing direction of one point, normalised; cams: m x 3 f64 camera centres in observation order."""
    p = [np.float64(np.float32(v)) for v in pos_f32]
    S = [np.float64(0.0)] * 3
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in np.asarray(cams, np.float64).reshape(-1, 3):
            d = [p[r] - c[r] for r in range(3)]
            s = d[0] * d[0]
            s = s + d[1] * d[1]
            s = s + d[2] * d[2]
            q = np.sqrt(s)
            for r in range(3):
                S[r] = S[r] + d[r] / q
        t = S[0] * S[0]
        t = t + S[1] * S[1]
        t = t + S[2] * S[2]
        q = np.sqrt(t)
        return np.array([S[r] / q for r in range(3)], np.float64)


def refresh(pos, desc, obs_desc, obs_cam, obs_start):
    """-> (choice n int32, desc n x 32 after the refresh, norm n x 3 f64).  A point without observations keeps its descriptor,
    choice -1, norm (0, 0, 0)."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    out_desc = np.array(desc, np.uint8).reshape(-1, 32)
    obs_desc = np.asarray(obs_desc, np.uint8).reshape(-1, 32)
    obs_cam = np.asarray(obs_cam, np.float64).reshape(-1, 3)
    n = len(pos)
    assert len(obs_start) == n + 1 and obs_start[0] == 0 and obs_start[n] == len(obs_desc)
    choice, norm = np.full(n, -1, np.int32), np.zeros((n, 3), np.float64)
    for i in range(n):
        a, b = int(obs_start[i]), int(obs_start[i + 1])
        assert 0 <= b - a <= MAX_OBS
        if a == b:
            continue
        choice[i] = medoid(obs_desc[a:b])[0]
        out_desc[i] = obs_desc[a + choice[i]]
        norm[i] = normal(pos[i], obs_cam[a:b])
    return choice, out_desc, norm


def tie_decided(obs_desc, obs_start, i):
    """Whether the minimal median of point i is reached by more than one observation (the index decides)."""
    a, b = int(obs_start[i]), int(obs_start[i + 1])
    if b - a < 2:
        return False
    med = medians(np.asarray(obs_desc, np.uint8).reshape(-1, 32)[a:b])
    return int((med == med.min()).sum()) > 1


def same_f64(a, b):
    """Equal by their bits, a NaN equal to any NaN (IEEE leaves the sign and payload of a generated NaN to the machine)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))
