"""The phantom study's host side (csrc/native/phantom.cpp) without a GPU: the phantom file's reader (fp32 and fp64
values, default and given times, every refusal with the dataset it names), the scores from hand-made sums against the
NumPy restatement of models/phantom.py bit for bit (zero denominators included), and the /phantom group's names, types
and shapes as PhantomWriter lays them out."""
import numpy as np
import pytest

from mpi_cuda_sartsolver_amd.io.fixtures import write_phantom_file
from mpi_cuda_sartsolver_amd.ops import native

pytestmark = pytest.mark.skipif(not native().have_hdf5(), reason="HDF5 not available")

NV = 11
SCORES = ("rel_l2", "cosine", "total_ratio", "peak_ratio", "max_error", "inside_fraction")


def _value(n=3):
    rng = np.random.default_rng(5)
    v = rng.random((n, NV))
    v[0, ::2] = 0.0
    v[n - 1] = 0.0  # an all-zero phantom is allowed: the dark frame
    return v


@pytest.mark.parametrize("dtype, stored", [(np.float64, "<f8"), (np.float32, "<f4")])
def test_reads_fp32_and_fp64_with_default_times(tmp_path, dtype, stored):
    v = _value()
    p = write_phantom_file(str(tmp_path / "p.h5"), v, dtype=dtype)
    assert native().dataset_dtype(p, "phantom/value") == stored
    value, time = native().read_phantom_file(p, NV)
    assert value.dtype == np.float64 and np.array_equal(value, v.astype(dtype).astype(np.float64))
    assert np.array_equal(time, [0.0, 1.0, 2.0])


def test_given_times(tmp_path):
    t = [0.125, 0.25, 7.0]
    _, time = native().read_phantom_file(write_phantom_file(str(tmp_path / "p.h5"), _value(), time=t), NV)
    assert np.array_equal(time, t)


def _refused(path, dataset, words):
    with pytest.raises(RuntimeError) as e:
        native().read_phantom_file(path, NV)
    msg = str(e.value)
    assert dataset in msg and words in msg and path in msg, msg


def test_refuses_a_missing_dataset(tmp_path):
    p = str(tmp_path / "lap.h5")
    native().write_laplacian_file(p, NV, np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.ones(1, np.float32))
    _refused(p, "phantom/value", "has no dataset")


def test_refuses_the_wrong_voxel_count(tmp_path):
    _refused(write_phantom_file(str(tmp_path / "p.h5"), np.ones((2, NV + 1))), "phantom/value",
             f"{NV + 1} voxels per row, the RTM has {NV}")


def test_refuses_no_phantom(tmp_path):
    _refused(write_phantom_file(str(tmp_path / "p.h5"), np.zeros((0, NV))), "phantom/value", "n = 0")


@pytest.mark.parametrize("bad", [-1e-300, -1.0, np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_refuses_negative_and_non_finite_entries(tmp_path, bad, dtype):
    v = _value()
    v[1, 4] = -1.0 if (dtype is np.float32 and bad == -1e-300) else bad  # (-1e-300 is -0 in fp32, which is allowed)
    _refused(write_phantom_file(str(tmp_path / "p.h5"), v, dtype=dtype), "phantom/value",
             "negative or non-finite entry (row 1, voxel 4)")


@pytest.mark.parametrize("t", [[0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 2.0], [0.0, 1.0, np.inf]])
def test_refuses_times_that_do_not_increase(tmp_path, t):
    _refused(write_phantom_file(str(tmp_path / "p.h5"), _value(), time=t), "phantom/time", "strictly increasing")


def test_scores_match_the_numpy_restatement_bit_for_bit():
    from mpi_cuda_sartsolver_amd.models.phantom import SCORE_NAMES, SUM_NAMES, phantom_scores

    assert tuple(SCORE_NAMES) == SCORES == tuple(native().phantom_score_names) and len(SUM_NAMES) == 10
    rng = np.random.default_rng(11)
    sums = rng.random((5, 40, 10)) * 10.0 ** rng.integers(-8, 9, size=(5, 40, 10))
    # zero denominators, each alone and together: s_t, s_tt, s_xx, s_x, m_t; then tiny and huge products
    for i, cols in enumerate(([0], [2], [3], [1], [8], [0, 2, 8], [0, 1, 2, 3, 8], list(range(10)))):
        sums[0, i, cols] = 0.0
    sums[1, 0, [2, 3]] = 1e-200  # the product underflows to 0: NaN by the zero-denominator rule
    sums[1, 1, [2, 3]] = 1e200   # the product overflows: a division by inf
    sums[1, 2, 5] = 0.0          # x == t
    got = native().phantom_scores(sums)
    want = phantom_scores(sums)
    assert got.shape == (5, 40, 6)
    for i, name in enumerate(SCORES):
        assert want[name].shape == (5, 40)
        assert np.array_equal(got[..., i], want[name], equal_nan=True), name
    # hand values: s_t s_x s_tt s_xx s_xt s_dd s_in m_d m_t m_x
    one = native().phantom_scores(np.array([4, 3, 8, 2, 3, 4, 2.5, 1.5, 2, 1], dtype=np.float64))
    assert np.array_equal(one, [np.sqrt(0.5), 3.0 / np.sqrt(16.0), 0.75, 0.5, 0.75, 2.5 / 3.0])
    dark = native().phantom_scores(np.array([0, 3, 0, 2, 0, 2, 0, 1, 0, 1], dtype=np.float64))
    assert np.all(np.isnan(dark[:5])) and dark[5] == 0.0
    assert np.isnan(got[1, 0, 1]) and got[1, 1, 1] == 0.0 and got[1, 2, 0] == 0.0


def test_writer_names_types_and_shapes(tmp_path):
    n, nc, npix = 3, 4, 7
    out = str(tmp_path / "o.h5")
    t = np.array([0.5, 1.5, 2.5])
    w = native().PhantomWriter(out, n, nc, npix, "truth.h5", t)
    rng = np.random.default_rng(2)
    sums = rng.random((n, nc, 10))
    for k in (2, 0, 1):  # any order
        w.write_phantom(k, sums[k], np.full(nc, -k, np.int32), np.arange(nc, dtype=np.int32) + k)
    image = rng.random((n, npix))
    w.write_images(image)
    rd, ty = native().read_dataset_f64, native().dataset_dtype
    shapes = {"image": (n, npix), "time": (n,), "sums": (n, nc, 10), "status": (n, nc), "iterations": (n, nc),
              **{s: (n, nc) for s in SCORES}}
    for name, shape in shapes.items():
        assert rd(out, "phantom/" + name).shape == shape, name
        assert ty(out, "phantom/" + name) == ("<i4" if name in ("status", "iterations") else "<f8"), name
    assert np.array_equal(rd(out, "phantom/image"), image) and np.array_equal(rd(out, "phantom/time"), t)
    assert np.array_equal(rd(out, "phantom/sums"), sums)
    assert np.array_equal(rd(out, "phantom/status"), -np.arange(n)[:, None] * np.ones(nc))
    assert np.array_equal(rd(out, "phantom/iterations"), np.arange(n)[:, None] + np.arange(nc)[None, :])
    scores = native().phantom_scores(sums)
    for i, name in enumerate(SCORES):
        assert np.array_equal(rd(out, "phantom/" + name), scores[..., i], equal_nan=True), name
    with pytest.raises(RuntimeError, match="out of bounds"):
        w.write_phantom(n, sums[0], np.zeros(nc, np.int32), np.zeros(nc, np.int32))
