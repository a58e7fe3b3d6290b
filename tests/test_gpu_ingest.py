"""On-device DPdataset transform (csrc/ingest.hip, latice.data_module) vs the restatement of
torchvision's ToPILImage -> Grayscale -> CenterCrop -> ToTensor (oracle/index_oracle.py):
bit-exact (integer uint8 path), over crop, odd-margin (round half to even) and pad cases."""
import numpy as np
import pytest
import torch

from latice import data_module as D
from oracle import index_oracle as IO

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H0,W0,out", [(160, 160, (128, 128)), (129, 131, (128, 128)),
                                        (133, 135, (128, 128)), (100, 140, (128, 128)),
                                        (128, 128, (128, 128)), (64, 61, (64, 64))])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ingest_matches_torchvision_restatement(cuda, H0, W0, out, dtype):
    rng = np.random.default_rng(H0 * 7 + W0)
    raw = rng.random((5, H0, W0)).astype(dtype)
    raw[0, :3, :3] = [[1.0, 0.0, -0.5], [1.5, np.nan, 0.999999], [1 / 255, 2 / 255, 0.5]]
    got = D.ingest_patterns(raw, out).cpu().numpy()
    assert np.array_equal(got, IO.ingest_patterns(raw, out))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).tobytes()


# B = 2, the smallest shapes that take both geometries of the one ingest kernel: a crop (offsets
# 2 and 1), a crop whose margins are odd (2.5 -> 2 and 1.5 -> 2, half to even) and a zero pad
@pytest.mark.parametrize("H0,W0", [(20, 18), (21, 19), (12, 12)])
def test_one_kernel_converts_every_source_type(cuda, H0, W0):
    size = (16, 16)
    # float sources: random in [0, 1) with every special value inside the window of both patterns
    rng = np.random.default_rng(H0)
    raw = rng.random((2, H0, W0))
    cy, cx = H0 // 2, W0 // 2
    raw[:, cy, cx - 3:cx + 3] = [np.nan, np.inf, -np.inf, -0.5, 1.5, 1.0]
    raw[:, cy + 1, cx - 3:cx + 3] = [0.0, -0.0, 0.999999, 1 / 255, 254.999 / 255, 1e-300]
    for dtype in (np.float64, np.float32):
        src = raw.astype(dtype)
        want = IO.ingest_patterns(src, size)
        assert np.isfinite(want).all()
        assert _bits(D.ingest_patterns(src, size).cpu().numpy()) == _bits(want)
    # uint8: every value once inside the window (the whole 12 x 12 pattern leaves room for 144
    # values each, so the two patterns share them), against the oracle and the device on v / 255
    v = np.zeros((2, H0, W0), np.uint8)
    if H0 >= 16:
        t, l = round((H0 - 16) / 2), round((W0 - 16) / 2)
        v[0, t:t + 16, l:l + 16] = np.arange(256, dtype=np.uint8).reshape(16, 16)
        v[1] = 255 - v[0]
    else:
        v[:] = np.arange(2 * H0 * W0).reshape(2, H0, W0) % 256
    assert np.unique(v).size == 256
    got = D.ingest_patterns_u8(v, size).cpu().numpy()
    assert got.shape == (2, 1, 16, 16) and got.dtype == np.float32
    assert np.unique(got).size == 256
    assert _bits(got) == _bits(IO.ingest_patterns(v / 255.0, size))
    assert _bits(got) == _bits(D.ingest_patterns(v.astype(np.float64) / 255.0, size).cpu().numpy())


def test_dpdataset_batches(cuda, tmp_path):
    rng = np.random.default_rng(2)
    raw = rng.random((10, 140, 140))
    np.save(tmp_path / "p.npy", raw)
    with open(tmp_path / "a.txt", "w") as f:
        f.write("eu\n10\n")
        for i in range(10):
            f.write(f"{i}.5  {2 * i} {3 * i}\n")
    ds = D.DPdataset(tmp_path / "p.npy", tmp_path / "a.txt", (128, 128))
    assert len(ds) == 10
    x, ang = ds.batch([3, 7])
    assert x.shape == (2, 1, 128, 128) and x.is_cuda
    assert np.array_equal(x.cpu().numpy(), IO.ingest_patterns(raw[[3, 7]]))
    assert np.allclose(ang, [[3.5, 6, 9], [7.5, 14, 21]])
    n = sum(b[0].shape[0] for b in ds.iter_batches(4))
    assert n == 10
