"""GPU: the host-pointer entries of the ruler's units over one thread's state (csrc/sdr_ruler_shared.hpp
HostCall over HostBufs).  No kernel is under test here: what can go wrong is the reuse of the
thread's buffers by calls of different kinds and sizes, and the placement of several outputs in one
buffer.  So every test is a sequence of calls on one thread, and every result is compared BIT FOR BIT
with the same call's device form on tensors, computed beforehand."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import check, lib  # noqa: E402
from stereo_depth_ruler_amd.ruler import (MEASUREMENT_DTYPE, OBJECT_DTYPE, OBJECT_SCAN_DTYPE, OUT_OF_RANGE,  # noqa: E402
                                          PLANE_DTYPE, PLANE_SEARCH_ROUND_DTYPE, as_segments)
from stereo_depth_ruler_amd.sgbm import _Q  # noqa: E402
from test_gpu_handle_binding import Worker  # noqa: E402
from test_gpu_ruler import SENTINEL  # noqa: E402

Q = S.REFERENCE_Q
SEARCH = dict(max_planes=2, hypotheses=64, seed=5, min_inliers=16)
OBJECTS = dict(h_range=(-1048576.0, 1048576.0), max_diff=0.5, min_pixels=3, max_objects=8)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def ruler(profile=False):
    return sdr.Ruler(Q, radius=1, min_count=2, conf_min=0.4, profile=profile)


class Scene:
    """Maps of (F, H, W) with noise, holes, a confidence map and a label map, the queries of the
    eight calls on them, and each call's result from its device form (read-only)."""

    def __init__(self, F, H, W, s16, seed):
        rng = np.random.default_rng(seed)
        ys, xs = np.mgrid[0:H, 0:W]
        d = (30.0 + 0.05 * xs - 0.03 * ys)[None] + rng.normal(0, 0.4, (F, H, W))
        d[:, H // 3:H // 2 + 1, W // 4:W // 2 + 1] += 6.0  # something stands on the ramp
        d = (np.round(d * 16) / 16).astype(np.float32)
        d[rng.random((F, H, W)) < 0.12] = -1.0
        self.F, self.H, self.W = F, H, W
        self.d = (d * 16).astype(np.int16) if s16 else d
        self.conf = rng.random((F, H, W)).astype(np.float32)
        self.labels = rng.integers(0, 3, (F, H, W)).astype(np.uint8)
        self.xyz = rng.uniform(-50.0, 50.0, (F, H, W, 3)).astype(np.float32)
        self.xyz[0, 0, 0, 2] = np.inf
        f, whole = F - 1, (0, 0, W - 1, H - 1)
        self.segs = as_segments([(0, 0, 0, W - 1, H - 1), (f, W - 2, 1, 1, H - 2), (f, 3, H // 2, min(8, W - 1), H // 2)])
        self.rects = as_segments([(0,) + whole, (f, 1, 1, W - 2, H - 2), (0, 0, 0, 0, H - 1), (f, W, 0, 1, 1),
                                  (f, W // 2, 0, W - 1, H - 1)])
        self.regions = [(0,) + whole + (0, 1), (f, 1, 1, W - 2, H - 2, 1, -1)]
        self.object_region = (f,) + whole + (1, -1)
        self.points = [(0, 2, 2, 0), (f, W - 1, H - 1, 1), (0, W // 2, H // 2, 2), (f, W, 0, 0), (f, 4, 3, 7)]
        # the device forms; the plane records of the fit feed the calls that take planes, as host records
        t = dict(d=dev(self.d), conf=dev(self.conf), labels=dev(self.labels), xyz=dev(self.xyz))
        self.planes = ruler().fit_plane(t["d"], self.rects, conf=t["conf"], min_inliers=16)
        self.want = [op(self, t) for op in OPS]
        torch.cuda.synchronize()

    def host(self):
        return dict(d=self.d, conf=self.conf, labels=self.labels, xyz=self.xyz)


# The eight calls.  m: the maps, host arrays or tensors; the Ruler's methods take the host ABI on the
# first and the device ABI on the second.  Each returns a list of arrays.
def op_find_objects(s, m):
    objs, scan, lab = ruler().find_objects(m["d"], s.planes, s.object_region, labels=m["labels"], conf=m["conf"],
                                           labels_out=True, **OBJECTS)
    return [objs, np.asarray(scan).reshape(1), lab]


def op_measure_profile(s, m):
    return list(ruler(profile=True).measure(m["d"], s.segs, conf=m["conf"]))


def op_find_planes(s, m):
    r = ruler()
    if not torch.is_tensor(m["d"]):
        rec, count, rounds, lab = r.find_planes_full(m["d"], s.rects[0], conf=m["conf"], labels=True, **SEARCH)
        return [rec, np.array([count], np.int32), rounds, lab]
    rec, count, rounds, lab = r.find_planes_device(m["d"], s.rects[0], conf=m["conf"], labels=True, **SEARCH)
    return [rec.cpu().numpy().reshape(-1).view(PLANE_DTYPE), count.cpu().numpy(),
            rounds.cpu().numpy().reshape(-1).view(PLANE_SEARCH_ROUND_DTYPE), lab.cpu().numpy()]


def op_relief(s, m):
    return [ruler().relief(m["d"], s.planes, s.regions, labels=m["labels"], conf=m["conf"], quantiles=(100, 900))]


def op_measure_xyz(s, m):
    return [ruler().measure_xyz(m["xyz"], s.segs)]


def op_fit_plane(s, m):
    return [ruler().fit_plane(m["d"], s.rects, conf=m["conf"], min_inliers=16)]


def op_plane_distance(s, m):
    return [ruler().plane_distance(m["d"], s.planes, s.points, conf=m["conf"])]


def op_footprint(s, m):
    return [ruler().footprint(m["d"], s.planes, s.regions, labels=m["labels"], conf=m["conf"], grid=16, cell=8.0)]


OPS = [op_find_objects, op_measure_profile, op_find_planes, op_relief, op_measure_xyz, op_fit_plane,
       op_plane_distance, op_footprint]


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}, output {k}: {g.shape} {g.dtype} / {w.shape} {w.dtype}"
        assert np.array_equal(raw(g), raw(w)), f"{what}, output {k} differs from the device form's"


def host_op(scene, op):
    assert_same(op(scene, scene.host()), scene.want[OPS.index(op)], f"{op.__name__} on {scene.d.shape}")


@pytest.fixture(scope="module")
def scenes():
    """(dtype is int16) -> the three passes' scenes and the scene whose calls fill the buffers between."""
    return {s16: dict(first=Scene(2, 40, 70, s16, 1), small=Scene(1, 9, 11, s16, 2), large=Scene(2, 64, 96, s16, 3),
                      other=Scene(2, 33, 57, s16, 4)) for s16 in (False, True)}


def test_device_forms_have_something_to_say(scenes):
    """The references are no empty records: objects, planes and profiles were found (the 9 x 11 scene
    may be too small for some of that; it is there for its size)."""
    for s16 in (False, True):
        for name in ("first", "large", "other"):
            sc = scenes[s16][name]
            objs, scan, lab = sc.want[0]
            rec, count, rounds, plab = sc.want[2]
            assert len(objs) >= 1 and (lab != 255).any() and count[0] >= 1 and (plab != 255).any(), name
            assert np.isfinite(sc.want[1][1]).any() and sc.want[3][0]["n"][0] > 0 and sc.want[5][0]["flags"][0] == 1, name


@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
def test_host_calls_share_one_thread_state(scenes, s16):
    sc = scenes[s16]
    w = Worker()

    def fill():  # calls of other kinds on other maps: labels, a profile and records that are not the pass's
        host_op(sc["other"], op_find_objects)
        host_op(sc["other"], op_measure_profile)
        host_op(sc["other"], op_relief)

    def run():
        for name, order in (("first", OPS), ("small", OPS[::-1]), ("large", OPS)):
            fill()
            for op in order:
                host_op(sc[name], op)

    try:
        w.call(run)
    finally:
        w.exit()


def search_args(sc):
    r = ruler()
    _, _, a = r._host_maps(sc.d, sc.conf)
    p = r._search_params(SEARCH["max_planes"], SEARCH["hypotheses"], SEARCH["seed"], 3, 1.0, SEARCH["min_inliers"])
    return a, p, np.ascontiguousarray(sc.rects[:1])


def test_optional_outputs_through_the_raw_abi(scenes):
    sc = scenes[False]["first"]
    H, W, n = sc.H, sc.W, SEARCH["max_planes"]
    want_planes, want_count, want_rounds, want_lab = sc.want[2]

    def find_planes():
        a, p, reg = search_args(sc)
        for with_rounds, with_labels in ((True, True), (False, True), (True, False), (False, False)):
            rec, count = np.zeros(n, PLANE_DTYPE), np.full(1, -7, np.int32)
            rounds, lab = np.zeros(n, PLANE_SEARCH_ROUND_DTYPE), np.full((H, W), 77, np.uint8)
            check(lib().sdr_find_planes(*a, _Q(Q), ctypes.byref(p), reg.ctypes.data, rec.ctypes.data, count.ctypes.data,
                                        rounds.ctypes.data if with_rounds else None,
                                        lab.ctypes.data if with_labels else None))
            what = f"sdr_find_planes, rounds {with_rounds}, labels {with_labels}"
            assert_same([rec, count], [want_planes, want_count], what)
            assert_same([rounds], [want_rounds if with_rounds else np.zeros(n, PLANE_SEARCH_ROUND_DTYPE)], what)
            assert_same([lab], [want_lab if with_labels else np.full((H, W), 77, np.uint8)], what)

    def find_objects():
        objs, scan, lab = ruler().find_objects(sc.d, sc.planes, sc.object_region, labels=sc.labels, conf=sc.conf,
                                               labels_out=False, **OBJECTS)
        assert lab is None
        assert_same([objs, np.asarray(scan).reshape(1)], sc.want[0][:2], "sdr_find_objects without labels_out")
        assert objs.dtype == OBJECT_DTYPE and scan.dtype == OBJECT_SCAN_DTYPE

    def profile():
        cap = 6
        f = sc.F - 1
        segs = as_segments([(0, 2, 2, 5, 3), (f, 7, 7, 7, 7), (f, W, 0, 1, 1), (0, 9, 4, 5, 8)])  # 4, 1, -, 5 samples
        r = ruler(profile=True)
        buf = torch.full((len(segs), cap, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
        rec, _ = r.measure_device(dev(sc.d), segs, conf=dev(sc.conf), profile_out=buf)
        torch.cuda.synchronize()
        want_rec, want_prof = rec.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE), buf.cpu().numpy()
        _, _, a = r._host_maps(sc.d, sc.conf)
        p = r._params(cap)
        got_rec = np.zeros(len(segs), MEASUREMENT_DTYPE)
        got_prof = np.full((len(segs), cap, 4), SENTINEL, np.float32)
        check(lib().sdr_measure_disp(*a, _Q(Q), ctypes.byref(p), segs.ctypes.data, len(segs), got_rec.ctypes.data,
                                     got_prof.ctypes.data))
        assert_same([got_rec, got_prof], [want_rec, want_prof], "sdr_measure_disp with a profile buffer of cap 6")
        for k, samples in enumerate((4, 1, 0, 5)):
            assert (got_prof[k, samples:] == SENTINEL).all() and (got_prof[k, :samples] != SENTINEL).all(), k
        assert got_rec["flags"][2] & OUT_OF_RANGE

    w = Worker()
    try:
        for task in (find_planes, find_objects, profile):
            w.call(task)
    finally:
        w.exit()


def test_empty_calls_between_full_ones(scenes):
    """A K == 0 call of each batched entry writes nothing and leaves the next full call's result alone."""
    sc = scenes[False]["first"]
    r = ruler(profile=True)
    _, _, a = r._host_maps(sc.d, sc.conf)
    F, H, W = sc.d.shape
    pl = np.ascontiguousarray(sc.planes)
    P, Qc, L = len(pl), _Q(Q), lib()
    some = np.zeros((4, 8), np.int32)  # non-null rows that K == 0 must not read
    lab = sc.labels.ctypes.data
    params = [r._params(6), r._plane_params(3, 1.0, 16), r._point_params(), r._relief_params((100, 900), 0.0),
              r._footprint_params(8.0, 16, 4, None)]
    empties = [
        (op_measure_profile, lambda o: L.sdr_measure_disp(*a, Qc, ctypes.byref(params[0]), some.ctypes.data, 0, o, o)),
        (op_measure_xyz, lambda o: L.sdr_measure_xyz(sc.xyz.ctypes.data, W * 3, W * H * 3, W, H, F, some.ctypes.data, 0, o)),
        (op_fit_plane, lambda o: L.sdr_fit_planes(*a, Qc, ctypes.byref(params[1]), some.ctypes.data, 0, o)),
        (op_plane_distance, lambda o: L.sdr_plane_distance(*a, Qc, ctypes.byref(params[2]), pl.ctypes.data, P,
                                                           some.ctypes.data, 0, o)),
        (op_relief, lambda o: L.sdr_plane_relief(*a, lab, Qc, ctypes.byref(params[3]), pl.ctypes.data, P,
                                                 some.ctypes.data, 0, o)),
        (op_footprint, lambda o: L.sdr_plane_footprint(*a, lab, Qc, ctypes.byref(params[4]), pl.ctypes.data, P,
                                                       some.ctypes.data, 0, o)),
    ]

    def run():
        for op, empty in empties:
            host_op(sc, op)
            out = np.full(1024, 0x5A, np.uint8)
            check(empty(out.ctypes.data))
            assert (out == 0x5A).all(), f"the empty call after {op.__name__} wrote"
            host_op(sc, op)

    w = Worker()
    try:
        w.call(run)
    finally:
        w.exit()
