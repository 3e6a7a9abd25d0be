"""The objects of a region without a device: the structures' layout and defaults, every host guard
of the C ABI, the Python surface's argument checks, the restatement (tests/objects_ref.py) against
a plain flood fill, its identities and refusals, and the feature's scene (a box top and a hemisphere
on a tilted floor) measured with the restatements only."""
import ctypes
from collections import deque

import numpy as np
import pytest

import footprint_ref as FR
import objects_ref as OR
import plane_ref as PR
import plane_search_ref as SR
import relief_ref as LR
import stereo_depth_ruler_amd as sdr
from stereo_depth_ruler_amd import _lib, pipeline
from stereo_depth_ruler_amd import synthetic as S
from stereo_depth_ruler_amd.ruler import OBJECT_DTYPE, OBJECT_SCAN_DTYPE

Q = S.REFERENCE_Q
EYE = np.eye(4)


def test_struct_layout_and_defaults():
    P, O, C = _lib.ObjectParams, _lib.Object, _lib.ObjectScan
    assert (ctypes.sizeof(P), ctypes.sizeof(O), ctypes.sizeof(C)) == (64, 64, 64)
    assert (OBJECT_DTYPE.itemsize, OBJECT_SCAN_DTYPE.itemsize) == (64, 64)
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("min_disp", 0), ("conf_min", 4), ("h_lo", 8), ("h_hi", 12), ("max_diff", 16), ("connectivity", 20),
        ("min_pixels", 24), ("max_objects", 28), ("reserved", 32)]
    want = [("n", 0), ("root", 4), ("x0", 8), ("y0", 12), ("x1", 16), ("y1", 20), ("sum_x", 24), ("sum_y", 32),
            ("sum256", 40), ("h_min", 48), ("h_max", 52), ("flags", 56), ("reserved", 60)]
    assert [(n, getattr(O, n).offset) for n, _ in O._fields_] == want
    assert [(n, OBJECT_DTYPE.fields[n][1]) for n in OBJECT_DTYPE.names] == want
    want = [("flags", 0), ("area", 4), ("n_masked", 8), ("n_valid", 12), ("n", 16), ("n_components", 20),
            ("n_kept", 24), ("count", 28), ("largest_dropped", 32), ("frame", 36), ("plane", 40), ("label", 44),
            ("reserved", 48)]
    assert [(n, getattr(C, n).offset) for n, _ in C._fields_] == want
    assert [(n, OBJECT_SCAN_DTYPE.fields[n][1]) for n in OBJECT_SCAN_DTYPE.names] == want
    assert OR.OBJECT_DTYPE == OBJECT_DTYPE and OR.SCAN_DTYPE == OBJECT_SCAN_DTYPE
    assert (sdr.OBJECTS_VALID, sdr.OBJECTS_OUT_OF_RANGE, sdr.OBJECTS_NO_PLANE, sdr.OBJECTS_EMPTY,
            sdr.OBJECTS_TRUNCATED) == (1, 2, 4, 8, 16)
    assert (OR.VALID, OR.OUT_OF_RANGE, OR.NO_PLANE, OR.EMPTY, OR.TRUNCATED) == (1, 2, 4, 8, 16)
    assert (sdr.OBJECT_VALID, sdr.OBJECT_CUT) == (1, 2) == (OR.OBJECT_VALID, OR.OBJECT_CUT)
    L = _lib.lib()
    assert L.sdr_abi_version() == 4
    p = P(9.0, 9.0, 9.0, 9.0, 9.0, 9, 9, 9, (ctypes.c_int32 * 8)(*[9] * 8))
    L.sdr_object_params_default(ctypes.byref(p))
    assert (p.min_disp, p.conf_min, p.h_lo, p.h_hi, p.max_diff, p.connectivity, p.min_pixels, p.max_objects) == (
        -1.0, 0.0, 10.0, 1048576.0, 1.0, 8, 64, 16)
    assert list(p.reserved) == [0] * 8
    L.sdr_object_params_default(None)


def test_host_guards_without_a_device():
    L = _lib.lib()
    Qc = (ctypes.c_double * 16)(*np.asarray(Q).reshape(16))
    ptr = ctypes.c_void_p(4096)  # never dereferenced: the guards return first
    W, H, F = 8, 6, 2

    def params(lo=10.0, hi=1048576.0, md=1.0, conn=8, minpx=64, maxo=16, res=(0,) * 8):
        return _lib.ObjectParams(-1.0, 0.0, lo, hi, md, conn, minpx, maxo, (ctypes.c_int32 * 8)(*res))

    def dev(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, lab_in=None, q=Qc, par=params(), planes=ptr, P=2,
            qs=ptr, objs=ptr, scan=ptr, lab_out=None):
        return L.sdr_find_objects_device(disp, typ, stride, fs, w, h, f, None, lab_in, q,
                                         ctypes.byref(par) if par else None, planes, P, qs, objs, scan, lab_out, None)

    def host(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, lab_in=None, q=Qc, par=params(), planes=ptr, P=2,
             qs=ptr, objs=ptr, scan=ptr, lab_out=None):
        return L.sdr_find_objects(disp, typ, stride, fs, w, h, f, None, lab_in, q,
                                  ctypes.byref(par) if par else None, planes, P, qs, objs, scan, lab_out)

    nan, inf = float("nan"), float("inf")
    for fn in (dev, host):
        assert fn(disp=None) == -1 and fn(q=None) == -1 and fn(par=None) == -1
        assert fn(qs=None) == -1 and fn(objs=None) == -1 and fn(scan=None) == -1 and fn(planes=None) == -1
        assert fn(w=0) == -1 and fn(h=0) == -1 and fn(f=0) == -1
        assert fn(stride=W - 1) == -1 and fn(fs=W * H - 1) == -1
        assert fn(typ=2) == -1 and fn(typ=-1) == -1
        assert fn(w=8193, stride=8193, fs=8193 * H) == -1 and fn(h=8193, fs=W * 8193) == -1
        assert fn(w=8192, stride=8192, h=4096, fs=8192 * 4096) == -1  # 2^25 pixels
        assert fn(P=-1) == -1
        assert fn(lab_in=ptr, lab_out=ptr) == -1  # the output must not be the input
        assert fn(par=params(lo=nan)) == -1 and fn(par=params(hi=nan)) == -1 and fn(par=params(lo=1.0, hi=0.5)) == -1
        for md in (nan, inf, -inf, -1.0, -1e-30):
            assert fn(par=params(md=md)) == -1, md
        for conn in (0, 1, 6, -8, 9):
            assert fn(par=params(conn=conn)) == -1, conn
        for minpx in (0, -1, (1 << 24) + 1):
            assert fn(par=params(minpx=minpx)) == -1, minpx
        for maxo in (0, -1, 65):
            assert fn(par=params(maxo=maxo)) == -1, maxo
        for i in range(8):
            assert fn(par=params(res=tuple(int(j == i) for j in range(8)))) == -1
        assert L.sdr_last_error()
    # (what passes the guards goes on to the device: the GPU tests)


def test_python_surface_checks_arguments():
    r = sdr.Ruler(Q)
    z = np.zeros((4, 4), np.float32)
    pl = np.zeros(1, sdr.PLANE_DTYPE)
    reg = [(0, 0, 0, 3, 3, 0, -1)]
    with pytest.raises(sdr.SDRError):
        r.find_objects(np.zeros((4, 4), np.float64), pl, reg)
    for bad in ([(0, 0, 3, 3)], [(0,) * 8], [(0.5, 0, 0, 3, 3)], [(0, 0, 0, 3, 3), (0, 0, 0, 3, 3)], []):
        with pytest.raises(sdr.SDRError):
            r.find_objects(z, pl, bad)
    with pytest.raises(sdr.SDRError):
        r.find_objects(z, pl, reg, conf=np.zeros((3, 4), np.float32))
    with pytest.raises(sdr.SDRError):
        r.find_objects(z, pl, reg, labels=np.zeros((4, 4), np.int32))
    with pytest.raises(sdr.SDRError):
        r.find_objects(z, pl, reg, labels=np.zeros((3, 4), np.uint8))
    for kw in (dict(h_range=(1.0, 0.0)), dict(h_range=(float("nan"), 1.0)), dict(max_diff=-1.0),
               dict(max_diff=float("inf")), dict(max_diff=float("nan")), dict(connectivity=6), dict(connectivity=0),
               dict(min_pixels=0), dict(min_pixels=2 ** 24 + 1), dict(min_pixels=1.5), dict(max_objects=0),
               dict(max_objects=65), dict(max_objects=2.5)):
        with pytest.raises(sdr.SDRError):
            r.find_objects(z, pl, reg, **kw)
    with pytest.raises(sdr.SDRError):
        r.find_objects_device(z, pl, reg)
    with pytest.raises(RuntimeError, match="without ruler="):
        pipeline.LiveLoop.find_objects(type("L", (), {"ruler": None})(), None, None, None)


# ---- the restatement ----
def flat_plane(offset=0.0, normal=(0.0, 0.0, 1.0), flags=PR.OK):
    """With Q the identity and this record, hf is the float disparity itself."""
    p = np.zeros(1, PR.DTYPE)
    p["normal"], p["offset"], p["flags"] = normal, offset, flags
    return p


def flood(member, d, max_diff, connectivity):
    """A plain BFS flood fill: each member's root, -1 on the others."""
    rh, rw = member.shape
    nb = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    roots = np.full((rh, rw), -1, np.int64)
    md = np.float32(max_diff)
    for v0 in range(rh):
        for u0 in range(rw):
            if not member[v0, u0] or roots[v0, u0] >= 0:
                continue
            roots[v0, u0] = v0 * rw + u0  # row-major: the first pixel met is the component's smallest index
            todo = deque([(v0, u0)])
            while todo:
                v, u = todo.popleft()
                for dv, du in nb:
                    a, b = v + dv, u + du
                    if 0 <= a < rh and 0 <= b < rw and member[a, b] and roots[a, b] < 0 \
                            and abs(np.float32(d[v, u] - d[a, b])) <= md:
                        roots[a, b] = v0 * rw + u0
                        todo.append((a, b))
    return roots


def random_map(rng, H, W, levels, density):
    d = rng.integers(0, levels, (H, W)).astype(np.float32) * np.float32(0.75) + np.float32(20.0)
    member = rng.random((H, W)) < density
    return np.where(member, d, np.float32(-1.0)).astype(np.float32), member


def partition(roots):
    """The components as a set of frozensets of (v, u)."""
    out = {}
    for (v, u), r in np.ndenumerate(roots):
        if r >= 0:
            out.setdefault(int(r), set()).add((v, u))
    return {frozenset(s) for s in out.values()}


def test_restatement_against_a_flood_fill():
    rng = np.random.default_rng(11)
    for trial in range(24):
        H, W = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        d, member = random_map(rng, H, W, int(rng.integers(2, 7)), rng.uniform(0.3, 0.9))
        for conn in (4, 8):
            md = float(rng.choice([0.0, 0.75, 1.0, 1.5]))
            got = OR.components(member, d, md, conn)
            assert np.array_equal(got, flood(member, d, md, conn)), (trial, H, W, conn, md)
            objs, scan, lab, roots = OR.find_objects(d[None], flat_plane(), (0, 0, 0, W - 1, H - 1), EYE,
                                                     h_range=(0.0, 100.0), max_diff=md, connectivity=conn,
                                                     min_pixels=3, max_objects=5)
            assert np.array_equal(roots, got) and scan["n"] == member.sum()
            ids, sizes = np.unique(got[member], return_counts=True)
            keys = sorted(((-int(s), int(i)) for i, s in zip(ids, sizes) if s >= 3))
            assert scan["n_components"] == len(ids) and scan["n_kept"] == len(keys)
            assert [(-int(o["n"]), int(o["root"])) for o in objs[:scan["count"]]] == keys[:5]
            for k in range(scan["count"]):
                assert int((lab == k).sum()) == objs[k]["n"]
                assert np.array_equal(lab == k, got == objs[k]["root"])
            assert int((lab != 255).sum()) == int(objs["n"].sum())


def test_identities():
    rng = np.random.default_rng(5)
    for trial in range(8):
        H, W = int(rng.integers(3, 36)), int(rng.integers(3, 36))
        d, member = random_map(rng, H, W, 4, 0.6)
        for conn in (4, 8):
            base = partition(OR.components(member, d, 1.0, conn))
            # flipping or transposing the map permutes the partition only
            fl = partition(OR.components(member[:, ::-1], d[:, ::-1], 1.0, conn))
            assert {frozenset((v, W - 1 - u) for v, u in s) for s in fl} == base
            ud = partition(OR.components(member[::-1], d[::-1], 1.0, conn))
            assert {frozenset((H - 1 - v, u) for v, u in s) for s in ud} == base
            tr = partition(OR.components(member.T.copy(), d.T.copy(), 1.0, conn))
            assert {frozenset((u, v) for v, u in s) for s in tr} == base
            # components at a smaller max_diff refine those at a larger one
            fine = partition(OR.components(member, d, 0.75, conn))
            assert all(any(s <= b for b in base) for s in fine) and len(fine) >= len(base)
        # 4-components refine 8-components
        p4, p8 = partition(OR.components(member, d, 1.0, 4)), partition(OR.components(member, d, 1.0, 8))
        assert all(any(s <= b for b in p8) for s in p4) and len(p4) >= len(p8)
        # sum(n) + the dropped pixels == scan.n (nothing truncated)
        objs, scan, lab, roots = OR.find_objects(d[None], flat_plane(), (0, 0, 0, W - 1, H - 1), EYE,
                                                 h_range=(0.0, 100.0), min_pixels=4, max_objects=64)
        ids, sizes = np.unique(roots[roots >= 0], return_counts=True)
        assert not scan["flags"] & OR.TRUNCATED
        assert int(objs["n"].sum()) + int(sizes[sizes < 4].sum()) == scan["n"]
        assert scan["largest_dropped"] == (int(sizes[sizes < 4].max()) if (sizes < 4).any() else 0)


def test_refusal_records_of_the_restatement():
    d = np.full((2, 6, 8), 5.0, np.float32)
    pl = np.concatenate([flat_plane(), flat_plane(flags=PR.DEGENERATE)])
    kw = dict(h_range=(0.0, 10.0), min_pixels=1, max_objects=3, min_disp=-3e38)
    for reg, flag, area in (((2, 0, 0, 7, 5, 0, -1), OR.OUT_OF_RANGE, 0), ((0, 0, 0, 8, 5, 0, -1), OR.OUT_OF_RANGE, 0),
                            ((0, 0, 0, 7, 5, 0, 3), OR.OUT_OF_RANGE, 0), ((0, 0, 0, 7, 5, 0, 256), OR.OUT_OF_RANGE, 0),
                            ((0, 0, 0, 7, 5, -1, -1), OR.NO_PLANE, 48), ((0, 0, 0, 7, 5, 2, -1), OR.NO_PLANE, 48),
                            ((1, 7, 5, 0, 0, 1, -1), OR.NO_PLANE, 48)):
        objs, scan, lab, roots = OR.find_objects(d, pl, reg, EYE, **kw)
        assert scan["flags"] == flag and scan["area"] == area and roots is None
        assert (scan["frame"], scan["plane"], scan["label"]) == (reg[0], reg[5], reg[6])
        assert all(scan[n] == 0 for n in ("n_masked", "n_valid", "n", "n_components", "n_kept", "count"))
        assert (lab == 255).all() and (objs["n"] == 0).all() and (objs["root"] == -1).all()
        assert (objs["x0"] == -1).all() and np.isnan(objs["h_min"]).all() and (objs["flags"] == 0).all()
    objs, scan, lab, _ = OR.find_objects(d, pl, (1, 7, 5, 0, 0, 0, -1), EYE, **kw)
    assert scan["flags"] == OR.VALID and scan["count"] == 1 and objs["n"][0] == 48 and objs["flags"][0] == 3
    assert (objs["x0"][0], objs["y0"][0], objs["x1"][0], objs["y1"][0]) == (0, 0, 7, 5)
    assert objs["sum_x"][0] == 6 * 28 and objs["sum_y"][0] == 8 * 15 and objs["sum256"][0] == 48 * 5 * 256
    # members, none kept: EMPTY with the counts as found
    objs, scan, lab, _ = OR.find_objects(d, pl, (0, 0, 0, 7, 5, 0, -1), EYE, **dict(kw, min_pixels=49))
    assert scan["flags"] == OR.EMPTY and (scan["n"], scan["n_components"], scan["n_kept"]) == (48, 1, 0)
    assert scan["largest_dropped"] == 48 and (lab == 255).all()
    # more kept than max_objects: TRUNCATED
    d2 = np.full((1, 3, 9), -1.0, np.float32)
    d2[0, 1, ::2] = 5.0
    objs, scan, lab, _ = OR.find_objects(d2, pl, (0, 0, 0, 8, 2, 0, -1), EYE, **kw)
    assert scan["flags"] == OR.VALID | OR.TRUNCATED and (scan["n_kept"], scan["count"]) == (5, 3)
    assert objs["root"].tolist() == [9, 11, 13] and objs["flags"].tolist() == [3, 1, 1]  # x = 0 is the border


# ---- the scene: a 150 x 100 mm box top and a 60 mm hemisphere on the tilted floor in a 320 x 240
# window of the reference view, sigma 0.15 px, 20 % holes, 5 % outliers ----
def scene():
    Qw = FR.scene_q(Q)
    d, truth, info = OR.two_object_scene(Qw)
    return Qw, d, truth, info


def scene_floor(Qw, d, truth):
    H, W = truth.shape
    planes, count, _, labels = SR.find_planes(d, (0, 0, 0, W - 1, H - 1), Qw, max_planes=3, hypotheses=256,
                                              min_inliers=1000, seed=0)
    floor_i = int(np.argmax([((labels == i) & (truth == 0)).sum() for i in range(count)]))
    return planes, floor_i


def purity_recall(lab, k, truth, t):
    hit = int(((lab == k) & (truth == t)).sum())
    return hit / int((lab == k).sum()), hit / int((truth == t).sum())


def test_two_objects_on_the_found_floor():
    """Measured here (printed below) with h_range (10, 1000), max_diff 1.0, connectivity 8, min_pixels 64:
    two kept objects; the box 3445 pixels, purity 0.9988, recall 1.0000; the hemisphere 2065 pixels,
    purity 0.9985, recall 0.9140 (its rim lies below 10 mm); the largest dropped component 2 pixels;
    with connectivity 4 the box's recall is 0.9878."""
    Qw, d, truth, info = scene()
    H, W = truth.shape
    # conditions, before anything else: neither object touches the window's edge
    for m in (info["box"], info["ball"]):
        assert m.any() and not (m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any())
    planes, floor_i = scene_floor(Qw, d, truth)
    whole = (0, 0, 0, W - 1, H - 1, floor_i, -1)
    kw = dict(h_range=(10.0, 1000.0), max_diff=1.0, min_pixels=64)
    objs, scan, lab, _ = OR.find_objects(d, planes, whole, Qw, connectivity=8, **kw)
    box_k, ball_k = (int(np.argmax([((lab == k) & (truth == t)).sum() for k in range(scan["count"])])) for t in (1, 2))
    pb, rb = purity_recall(lab, box_k, truth, 1)
    ps, rs = purity_recall(lab, ball_k, truth, 2)
    objs4, scan4, lab4, _ = OR.find_objects(d, planes, whole, Qw, connectivity=4, **kw)
    box4 = int(np.argmax([((lab4 == k) & (truth == 1)).sum() for k in range(scan4["count"])]))
    _, rb4 = purity_recall(lab4, box4, truth, 1)
    print("kept %d of %d components, largest dropped %d; box: %d px purity %.4f recall %.4f; hemisphere: %d px "
          "purity %.4f recall %.4f; connectivity 4: box recall %.4f"
          % (scan["n_kept"], scan["n_components"], scan["largest_dropped"], objs["n"][box_k], pb, rb,
             objs["n"][ball_k], ps, rs, rb4))
    assert scan["flags"] == OR.VALID and scan["n_kept"] == 2 and scan["count"] == 2 and {box_k, ball_k} == {0, 1}
    assert scan["largest_dropped"] < 64
    assert pb >= 0.99 and rb >= 0.99
    assert ps >= 0.99 and rs >= 0.85
    assert rb4 < 0.99
    assert not (objs["flags"][:2] & OR.OBJECT_CUT).any()
    # the label map is what the relief takes: its counts and sums are the records'
    for k in range(2):
        r = LR.relief(d, planes, [(0, 0, 0, W - 1, H - 1, floor_i, k)], Qw, labels=lab)[0]
        assert r["flags"] == LR.VALID and r["n"] == objs["n"][k] and r["sum256"] == objs["sum256"][k]
        assert r["h_min"] == objs["h_min"][k] and r["h_max"] == objs["h_max"][k]
