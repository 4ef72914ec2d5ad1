"""Known answers, worked by hand, of the numpy transcription of the map-point refresh (tests/map_refresh_numpy.py): what the
MI355X kernel and the emulated build are then compared with bit for bit (tests/test_gpu_map_refresh.py,
tests/test_map_refresh_sim.py)."""
import numpy as np

import map_refresh_numpy as R


def bits(*ranges):
    """A 32-byte descriptor with the bits of the given half-open ranges set."""
    b = np.zeros(256, np.uint8)
    for lo, hi in ranges:
        b[lo:hi] = 1
    return np.packbits(b)


def thermo(x):
    """The first x bits set: the Hamming distance of thermo(a) and thermo(b) is |a - b|."""
    return bits((0, x))


def test_three_observations_at_distances_10_20_30():
    A, B, C = bits(), bits((0, 10)), bits((10, 30))          # |AB| = 10, |AC| = 20, |BC| = 30
    assert R.hamming([A, B, C], [A, B, C]).tolist() == [[0, 10, 20], [10, 0, 30], [20, 30, 0]]
    # rows sorted: A (0, 10, 20), B (0, 10, 30), C (0, 20, 30); index (3 - 1) // 2 = 1
    choice, med = R.medoid([A, B, C])
    assert med.tolist() == [10, 10, 20] and choice == 0      # A and B tie: the lower index
    choice, med = R.medoid([C, B, A])
    assert med.tolist() == [20, 10, 10] and choice == 1


def test_one_and_two_observations():
    choice, med = R.medoid([thermo(77)])
    assert med.tolist() == [0] and choice == 0
    # two: each row is (0, d), index (2 - 1) // 2 = 0: both medians are 0, observation 0 wins
    choice, med = R.medoid([thermo(3), thermo(200)])
    assert med.tolist() == [0, 0] and choice == 0


def test_even_count_takes_the_lower_median():
    """Four observations on a line at 0, 1, 10, 30.  Rows sorted: (0, 1, 10, 30), (0, 1, 9, 29), (0, 9, 10, 20), (0, 20, 29, 30).
    Index (4 - 1) // 2 = 1, the LOWER median: 1, 1, 9, 20 -> observation 0.  The upper median (index 2) would read 10, 9, 10, 29
    and choose observation 1."""
    d = [thermo(x) for x in (0, 1, 10, 30)]
    choice, med = R.medoid(d)
    assert med.tolist() == [1, 1, 9, 20] and choice == 0
    assert np.sort(R.hamming(d, d), axis=1)[:, 2].tolist() == [10, 9, 10, 29]


def test_duplicated_observations_tie_and_the_lower_index_wins():
    d = [thermo(5), thermo(0), thermo(0)]                     # rows sorted: (0, 5, 5), (0, 0, 5), (0, 0, 5)
    choice, med = R.medoid(d)
    assert med.tolist() == [5, 0, 0] and choice == 1
    assert R.tie_decided(np.array(d), [0, 3], 0)
    # five on a line at 0, 10, 11, 13, 30: rows sorted (0, 10, 11, 13, 30), (0, 1, 3, 10, 20), (0, 1, 2, 11, 19), (0, 2, 3, 13, 17),
    # (0, 17, 19, 20, 30); index 2 reads 11, 3, 2, 3, 19: one minimum, no tie
    line = np.array([thermo(x) for x in (0, 10, 11, 13, 30)])
    assert R.medoid(line)[1].tolist() == [11, 3, 2, 3, 19] and R.medoid(line)[0] == 2 and not R.tie_decided(line, [0, 5], 0)


def test_normal_of_two_symmetric_cameras_is_exactly_the_axis():
    """Point (0, 0, 2), cameras (-1, 0, 0) and (1, 0, 0): the directions are (+-1, 0, 2) / sqrt(5); the x components cancel
    exactly, S = (0, 0, z + z) and sqrt(fl(Sz Sz)) = Sz in binary floating point, so the result is (0, 0, 1) to the bit."""
    n = R.normal(np.float32([0, 0, 2]), [[-1, 0, 0], [1, 0, 0]])
    assert n.tobytes() == np.float64([0, 0, 1]).tobytes()
    n = R.normal(np.float32([0, 0, 2]), [[0, 0, 5]])          # a single camera behind the point: its own direction
    assert n.tobytes() == np.float64([0, 0, -1]).tobytes()
    # the position is the f32 value widened, not a decimal: 0.1f is 0.100000001490116...
    n = R.normal(np.float32([0.1, 0, 0]), [[0, 0, 0]])
    assert n.tobytes() == np.float64([1, 0, 0]).tobytes()


def test_camera_at_the_point_gives_nan():
    assert np.isnan(R.normal(np.float32([1, 2, 3]), [[1, 2, 3]])).all()
    assert np.isnan(R.normal(np.float32([1, 2, 3]), [[0, 0, 0], [1, 2, 3]])).all()   # one such observation spoils the sum
    assert R.same_f64([np.nan, 1.0], [-np.nan, 1.0]) and not R.same_f64([0.0], [-0.0]) and not R.same_f64([np.nan], [1.0])


def test_refresh_with_and_without_observations():
    pos = np.float32([[0, 0, 2], [5, 5, 5], [0, 0, 2]])
    desc = np.stack([thermo(100), thermo(101), thermo(102)])
    obs_desc = np.stack([thermo(5), thermo(0), thermo(0), thermo(9), thermo(8)])
    obs_cam = np.float64([[-1, 0, 0], [1, 0, 0], [0, 0, 0], [-1, 0, 0], [1, 0, 0]])
    choice, out, norm = R.refresh(pos, desc, obs_desc, obs_cam, [0, 3, 3, 5])
    assert choice.tolist() == [1, -1, 0] and choice.dtype == np.int32
    assert out[0].tobytes() == thermo(0).tobytes() and out[1].tobytes() == thermo(101).tobytes() and out[2].tobytes() == thermo(9).tobytes()
    assert norm[1].tolist() == [0, 0, 0] and norm[2].tobytes() == np.float64([0, 0, 1]).tobytes()
    assert norm[0, 1] == 0 and norm[0, 2] > 0.9 and abs(np.linalg.norm(norm[0]) - 1) < 1e-15
    assert desc[0].tobytes() == thermo(100).tobytes()         # (the input is left alone)
    choice, out, norm = R.refresh(pos, desc, np.zeros((0, 32), np.uint8), np.zeros((0, 3)), [0, 0, 0, 0])
    assert choice.tolist() == [-1, -1, -1] and out.tobytes() == desc.tobytes() and not norm.any()
