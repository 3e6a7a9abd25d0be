"""The path-cost record formats of the chain path (k_paths -> k_south_wta): int16 L, or 12-bit
e = C - L (0 <= e <= P2 <= 4095; include/sdr/sdr.h, sdr_sgbm_debug_stage).  The consumer rebuilds
L = C - e exactly, so both formats give the oracle's map bit for bit; a matcher created with
SDR_PATH_REC=16 in the environment keeps int16 records.
"""
import ctypes
import os
from contextlib import contextmanager

import numpy as np
import pytest

import path_cases
import stereo_depth_ruler_amd as sdr
from stereo_depth_ruler_amd import _lib
from stereo_depth_ruler_amd import synthetic as S
from test_oracle_sgm_volume import p2_domain_max

D = 128


@contextmanager
def path_rec_env(value):
    old = os.environ.get("SDR_PATH_REC")
    if value is None:
        os.environ.pop("SDR_PATH_REC", None)
    else:
        os.environ["SDR_PATH_REC"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SDR_PATH_REC", None)
        else:
            os.environ["SDR_PATH_REC"] = old


def create(args, rec16):
    """A matcher with the default record format, or one created under SDR_PATH_REC=16."""
    with path_rec_env("16" if rec16 else None):
        return sdr.StereoSGBM.create(*args)


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_pairs, _refs = {}, {}


def noisy_pair(H, W, seed):
    """Seeded texture + disparity shift + strong noise: matches and mismatches, e over [0, P2]."""
    key = (H, W, seed)
    if key not in _pairs:
        L, R, _ = S.make_pair(H, W, D, seed=seed, noise=12.0)
        _pairs[key] = (L, R)
    return _pairs[key]


def reference(oracle, tag, L, R, args):
    """(final map, LR-checked map) of the oracle, computed once per case."""
    key = (tag, args)
    if key not in _refs:
        p = oracle.make_params(*args)
        _refs[key] = (oracle.sgbm_compute(L, R, p), oracle.sgbm_compute(L, R, oracle.make_params(*args), stages=0))
    return _refs[key]


def check_both_formats(oracle, tag, L, R, args):
    ref, ref_lr = reference(oracle, tag, L, R, args)
    H, W = L.shape
    for rec16 in (False, True):
        m = create(args, rec16)
        got = m.compute(L, R)
        assert np.array_equal(got, ref), f"rec16={rec16}: {(got != ref).sum()} px differ"
        assert np.array_equal(m.debug_stage(2, (H, W), np.int16), ref_lr), f"rec16={rec16}: LR-checked map"
        m.close()


def sgbm_args(P1, P2, mode=0):
    # (minD, D, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniqueness, speckle ws, range, mode)
    return (0, D, 5, P1, P2, 1, 63, 12, 0, 0, mode)


# W1 = W - D = 64, 77, 96: E/W chains of two or more ring periods (32 steps) plus a tail, diagonals of
# every length from 1; H = 40, 37, 25: a partial last block of k_south_wta's 12 rows
SIZES = [(192, 40), (205, 37), (224, 25)]


@pytest.mark.gpu
@pytest.mark.parametrize("P1", [600, 4000])
@pytest.mark.parametrize("P2", [2400, 4095])
@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sgbm_both_formats_match_oracle(gpu, oracle, W, H, P2, P1):
    L, R = noisy_pair(H, W, seed=W + H)
    check_both_formats(oracle, ("sgbm", W, H), L, R, sgbm_args(P1, P2))


@pytest.mark.gpu
@pytest.mark.parametrize("P2", [4096, p2_domain_max(5, 63, 0)], ids=["P2_4096", "P2_domain_max"])
def test_p2_above_12_bits_falls_back(gpu, oracle, P2):
    W, H = 192, 40
    L, R = noisy_pair(H, W, seed=W + H)
    args = sgbm_args(600, P2)
    check_both_formats(oracle, ("sgbm", W, H), L, R, args)
    # the default matcher wrote int16 records too: the same bytes as the int16 matcher's
    n = H * (W - D) * 4 * D
    recs = []
    for rec16 in (False, True):
        m = create(args, rec16)
        m.compute(L, R)
        recs.append(m.debug_stage(4, (n,), np.int16))
        m.close()
    assert np.array_equal(recs[0], recs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 3], ids=["HH", "HH4"])
def test_hh_chain_path_both_formats(gpu, oracle, mode):
    """One frame of MODE_HH (below the sweep's batch size: chains, 7 records) on independent noise
    with P2 = 4095: eight paths' sum saturates at 32767 where five paths' does not; MODE_HH4: 3."""
    W, H = 192, 40
    L, R = S.adversarial_pair("noise", H, W, D, seed=11)
    check_both_formats(oracle, ("hh-noise", W, H), L, R, sgbm_args(600, 4095, mode))


@pytest.mark.gpu
def test_two_frame_batch(gpu, oracle):
    torch = gpu
    W, H = 205, 37
    args = sgbm_args(600, 2400)
    pairs = [noisy_pair(H, W, seed=W + H), noisy_pair(H, W, seed=5)]
    Ld = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    Rd = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    for rec16 in (False, True):
        m = create(args, rec16)
        got = m.compute(Ld, Rd)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        lr = m.debug_stage(2, (2, H, W), np.int16)
        for f, (L, R) in enumerate(pairs):
            ref, ref_lr = reference(oracle, ("sgbm", W, H, f), L, R, args)
            assert np.array_equal(got[f], ref), f"rec16={rec16} frame {f}"
            assert np.array_equal(lr[f], ref_lr), f"rec16={rec16} frame {f}: LR-checked map"
        m.close()


def decode_rec12(raw, H, W1, nrec):
    """Stage 4's 12-bit records (sdr.h) -> e [H][W1][nrec][D]."""
    return path_cases.decode_rec12(raw, H, W1, nrec, D)


@pytest.mark.gpu
def test_record_round_trip(gpu):
    """C - e of the 12-bit matcher's records == L of the int16 matcher's, in all four directions:
    the producer's half of the format on its own (the oracle tests cover producer + consumer)."""
    W, H, nrec = 192, 40, 4
    W1 = W - D
    L, R = noisy_pair(H, W, seed=W + H)
    args = sgbm_args(600, 2400)
    m16 = create(args, True)
    m16.compute(L, R)
    C = m16.debug_stage(0, (H, W1, D), np.int16).astype(np.int64)
    L16 = m16.debug_stage(4, (H, W1, nrec, D), np.int16).astype(np.int64)
    m16.close()
    m12 = create(args, False)
    m12.compute(L, R)
    raw = m12.debug_stage(4, (H * W1 * nrec * (D // 8) * 3,), np.uint32)
    m12.close()
    e = decode_rec12(raw, H, W1, nrec)
    assert e.min() >= 0 and e.max() <= 2400
    assert e.max() == 2400  # a chain's first pixel
    for q, name in enumerate(("E", "W", "SE", "SW")):
        bad = (C - e[:, :, q, :]) != L16[:, :, q, :]
        assert not bad.any(), f"direction {name}: {bad.sum()} values differ"


@pytest.mark.gpu
def test_handle_creation_under_either_value(gpu):
    for v in (None, "16", "12", "junk"):
        with path_rec_env(v):
            sdr.StereoSGBM.create(*sgbm_args(600, 2400)).close()


def test_scratch_bytes_unchanged_for_c2():
    """The records keep their int16 allocation: sdr_sgbm_scratch_bytes of the benchmark's default
    workload (1280x720, d = 128, MODE_SGBM) is what the int16 layout needs, under either setting."""
    W, H, P = 1280, 720, 5
    px, cells = W * H, H * (W - D) * D
    want = 3 * px * 4 + 3 * px * 8 + cells * 2 * P + px * 2 * 3 + px * 4 + px * 4 * 2
    assert want == 1111449600
    p = _lib.SgbmParams(0, D, 5, 600, 2400, 1, 63, 12, 200, 2, 0, 4, 0)
    for v in (None, "16"):
        with path_rec_env(v):
            for F in (1, 2, 4):
                assert _lib.lib().sdr_sgbm_scratch_bytes(ctypes.byref(p), W, H, F) == F * want
