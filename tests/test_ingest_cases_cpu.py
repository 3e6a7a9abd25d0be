"""The ingest edge cases (ingest_cases.py) without a GPU: conditions on the inputs of
test_gpu_ingest_edges.py, from the oracle alone, so that the GPU test cannot miss its target --
every zoom map holds every border class, the shift maps are what the closed form assumes, the
closed form is the oracle's answer, and the oracle's remap agrees with the numpy restatement."""
import os

import numpy as np
import pytest

import ingest_cases as C
import numpy_ref as NR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _src(case, eye, cn=3):
    f = C.sbs_frames(case.W, case.H)[0, :, eye * case.W:(eye + 1) * case.W]
    return np.ascontiguousarray(f if cn == 3 else f[..., 1])


def test_case_list_covers_what_it_claims():
    assert len({c.id for c in C.CASES}) == len(C.CASES)
    for W, H in C.SIZES:
        zs = [c for c in C.cases_of(W, H) if c.name.startswith("zoom")]
        assert sorted(len(c.eyes[0][1]) for c in zs) == sorted(C.NDIST)
        assert sorted(len(c.eyes[1][1]) for c in zs) == sorted(C.NDIST)
        for c in zs:
            assert len(c.eyes[0][1]) != len(c.eyes[1][1]) and c.eyes[0][3].shape == (3, 4)
            assert c.eyes[0][2][0, 1] == -c.eyes[1][2][0, 1] != 0
    assert any(w & 1 for w, h in C.SIZES_ODD) and any(h & 1 for w, h in C.SIZES_ODD)
    assert all(w % 2 == 0 and h % 2 == 0 for w, h in C.SIZES_EVEN)
    assert all(c.eyes[0][3].shape == (3, 3) for c in C.SHIFT_CASES)


def test_reference_calibration_border_classes(oracle):
    """Why these cases exist: the reference calibration's maps never leave the source but for a
    few right-eye entries on the bottom row."""
    from stereo_depth_ruler_amd.config import StereoConfiguration

    cfg = StereoConfiguration()
    assert cfg.loadFromFile(os.path.join(GOLDEN, "stereo.yaml"))
    W, H = cfg.imageSize
    for eye, (K, D, R, P) in enumerate(((cfg.cameraMatrixLeft, cfg.distCoeffsLeft, cfg.R1, cfg.P1),
                                        (cfg.cameraMatrixRight, cfg.distCoeffsRight, cfg.R2, cfg.P2))):
        m1, _ = oracle.init_undistort_rectify_map(K, D, R, P, W, H)
        n = C.classify(m1, W, H)
        assert n["outside"] == n["sx==-1"] == n["sx==W-1"] == n["sy==-1"] == 0, (eye, n)
        assert n["sy==H-1"] == (0 if eye == 0 else 21), (eye, n)


@pytest.mark.parametrize("case", [c for c in C.ZOOM_CASES if (c.W, c.H) not in C.TINY], ids=lambda c: c.id)
def test_zoom_maps_hold_every_border_class(oracle, case):
    for eye in (0, 1):
        m1, _ = C.oracle_maps(oracle, case, eye)
        n = C.classify(m1, case.W, case.H)
        for k in C.CLASSES:
            assert n[k] >= C.MIN_CLASS, (eye, k, n)
        # and the test needs a partial sum of every kind, not only entries that are outside anyway
        for k in C.CLASSES[:4]:
            assert n["partial:" + k] > 0, (eye, k, n)
        assert 4 * n["inside"] >= case.W * case.H, (eye, n)


def test_zoom_eyes_differ(oracle):
    for case in C.ZOOM_CASES:
        if (case.W, case.H) in C.TINY:
            continue
        l, r = C.oracle_maps(oracle, case, 0), C.oracle_maps(oracle, case, 1)
        assert not np.array_equal(l[0], r[0]), case.id


@pytest.mark.parametrize("case", C.SHIFT_CASES, ids=lambda c: c.id)
def test_shift_maps_and_closed_form(oracle, case):
    W, H = case.W, case.H
    sign = 1 if case.name == "shift+" else -1
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    for eye in (0, 1):
        m1, m2 = C.oracle_maps(oracle, case, eye)
        assert (m2 == 528).all()
        off = -1 if sign > 0 else 0
        assert np.array_equal(m1[..., 0], jj + off) and np.array_equal(m1[..., 1], ii + off)
        if sign > 0:
            assert (m1[:, 0, 0] == -1).all() and (m1[0, :, 1] == -1).all()
        else:
            assert (m1[:, -1, 0] == W - 1).all() and (m1[-1, :, 1] == H - 1).all()
        for cn in (1, 3):
            src = _src(case, eye, cn)
            assert np.array_equal(oracle.remap_bilinear(src, m1, m2), C.shift_closed_form(src, sign))


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_remap_equals_numpy(oracle, size):
    for case in C.cases_of(*size):
        for eye in (0, 1):
            m1, m2 = C.oracle_maps(oracle, case, eye)
            for cn in (1, 3):
                src = _src(case, eye, cn)
                assert np.array_equal(oracle.remap_bilinear(src, m1, m2), NR.remap_bilinear(src, m1, m2)), \
                    (case.id, eye, cn)
            # a source of another size than the map (sdr_remap_bilinear_device's case)
            src = _src(case, eye)[:max(1, case.H - 2), :max(1, case.W - 3)]
            src = np.ascontiguousarray(src)
            assert np.array_equal(oracle.remap_bilinear(src, m1, m2), NR.remap_bilinear(src, m1, m2))


def test_integer_formulas_equal_oracle(oracle):
    """The plain formulas test_gpu_post_entries.py uses as its second reference."""
    rng = np.random.default_rng(5)
    for W, H in ((2, 2), (254, 4), (258, 6), (90, 64)):
        bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        g = oracle.bgr2gray(bgr)
        assert np.array_equal(g, C.bgr2gray_int(bgr))
        assert np.array_equal(oracle.resize_area_half(g), C.area_half_int(g))
