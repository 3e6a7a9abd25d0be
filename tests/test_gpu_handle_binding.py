"""The host layer the auxiliary units share (csrc/sdr_host.hpp), BIT FOR BIT against the oracle:

* the handle base (sdr::Bound) of the display, the rectifier and the WLS filter: one call on the
  handle's own stream, on a caller's stream after set_stream, on the own stream again after
  reset_stream, then destroy;
* the per-thread state (sdr::ThreadState) of the host-pointer entries that take no handle,
  sdr_reproject and sdr_measure_xyz: two threads alternating, the first again after the second has
  exited, and, with two devices, the state following the thread's current device;
* the voxel grid over its planned arena at one point, past a block and past a sort tile.
"""
import ctypes
import queue
import threading
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import emit_cases as E  # noqa: E402
import ruler_ref as RR  # noqa: E402
from fgs_cases import hyp_case, make_filter  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import check, lib  # noqa: E402
from stereo_depth_ruler_amd.display import Display  # noqa: E402
from stereo_depth_ruler_amd.rectify import StereoRectifier  # noqa: E402
from stereo_depth_ruler_amd.ruler import MEASUREMENT_DTYPE  # noqa: E402
from stereo_depth_ruler_amd.sgbm import _cstream  # noqa: E402

W, H = 24, 16  # the binding tests' frame
TW, TH = 17, 9  # the per-thread tests' frame
Q = S.REFERENCE_Q


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


# ---- the handle base ---------------------------------------------------------------------------

def display_case(oracle):
    rng = np.random.default_rng(24)
    disp = rng.uniform(-4.0, 70.0, (H, W)).astype(np.float32)
    d = Display()
    d_disp, out = dev(disp), torch.empty((H, W), dtype=torch.uint8, device="cuda")

    def run():
        d.reset()  # the EMA history of the run before does not enter
        check(lib().sdr_show_disparity_map_device(d._h, d_disp.data_ptr(), W, H, W, W * H, 1, 64, out.data_ptr()))
        return [out]

    return d, lib().sdr_display_set_stream, lib().sdr_display_reset_stream, run, [oracle.show_disparity_map(disp, 64)]


def rectifier_case(oracle):
    rng = np.random.default_rng(16)
    K = np.array([[30.0, 0, W / 2 + 0.7], [0, 29.5, H / 2 - 0.4], [0, 0, 1]])
    a = 0.03
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    P = np.hstack([K * 1.05, [[3.0], [0.0], [0.0]]])
    P[2] = [0, 0, 1, 0]
    D = np.array([0.05, -0.02, 0.001, -0.002, 0.01])
    cfg = types.SimpleNamespace(imageSize=(W, H), cameraMatrixLeft=K, distCoeffsLeft=D, R1=R, P1=P,
                                cameraMatrixRight=K, distCoeffsRight=-D, R2=R.T, P2=P)
    r = StereoRectifier(cfg)
    L = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    Rt = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    dL, dR = dev(L), dev(Rt)
    lo, ro = torch.empty_like(dL), torch.empty_like(dR)

    def run():
        check(lib().sdr_rectify_device(r._h, dL.data_ptr(), dR.data_ptr(), W * 3, W * H * 3, 3, 1, lo.data_ptr(),
                                       ro.data_ptr(), W * 3, W * H * 3))
        return [lo, ro]

    ref = [oracle.remap_bilinear(src, *oracle.init_undistort_rectify_map(K, dist, Rm, P, W, H))
           for src, dist, Rm in ((L, D, R), (Rt, -D, R.T))]
    return r, lib().sdr_rectifier_set_stream, lib().sdr_rectifier_reset_stream, run, ref


def wls_case(oracle):
    g, dl, dr, q = hyp_case(oracle, np.random.default_rng(7), W, H, "noise", 8000.0, 1.5, D=8)
    f = make_filter(q, W, H)
    d_dl, d_dr, d_g = dev(dl), dev(dr), dev(g)
    out = torch.empty((H, W), dtype=torch.int16, device="cuda")
    conf = torch.empty((H, W), dtype=torch.float32, device="cuda")

    def run():
        check(lib().sdr_wls_filter_device(f._h, d_dl.data_ptr(), d_dr.data_ptr(), d_g.data_ptr(), W, H, W, W * H, 1,
                                          out.data_ptr(), conf.data_ptr()))
        return [out, conf]

    return f, lib().sdr_wls_set_stream, lib().sdr_wls_reset_stream, run, list(oracle.wls_filter(dl, dr, g, q, True))


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("case", [display_case, rectifier_case, wls_case], ids=["display", "rectifier", "wls"])
def test_own_stream_callers_stream_and_back(oracle, case):
    obj, set_stream, reset_stream, run, ref = case(oracle)
    got = []

    def collect(sync):
        outs = run()
        sync()
        got.append([o.cpu().numpy().copy() for o in outs])
        for o in outs:
            o.zero_()  # the next run writes every pixel again
        torch.cuda.synchronize()

    torch.cuda.synchronize()  # the inputs are there before a non-blocking stream reads them
    collect(torch.cuda.synchronize)  # the handle's own stream
    s = torch.cuda.Stream()
    check(set_stream(obj._h, ctypes.c_void_p(s.cuda_stream)))
    collect(s.synchronize)  # the caller's stream: its own synchronize is enough
    check(reset_stream(obj._h))
    collect(torch.cuda.synchronize)
    obj.close()
    assert obj._h is None
    for k, outs in enumerate(got):
        assert len(outs) == len(ref)
        for o, r in zip(outs, ref):
            assert o.shape == r.shape and o.dtype == r.dtype
            assert np.array_equal(raw(o), raw(r)), f"run {k} differs from the oracle"


# ---- the per-thread state --------------------------------------------------------------------------

def qptr():
    return (ctypes.c_double * 16)(*np.asarray(Q, np.float64).ravel())


@pytest.fixture(scope="module")
def thread_inputs(oracle):
    """disp (TH, TW) with one minimum, its reprojections for handle_missing 0 and 1, segments on the
    first of them and their records (read-only)."""
    rng = np.random.default_rng(179)
    disp = rng.uniform(2.0, 60.0, (TH, TW)).astype(np.float32)
    disp[3, 5] = -1.0
    xyz = {hm: E.ro(oracle.reproject(disp, Q, bool(hm))) for hm in (0, 1)}
    assert int((xyz[1][..., 2] == 10000.0).sum()) == 1
    segs = np.stack([np.zeros(12), rng.integers(0, TW, 12), rng.integers(0, TH, 12), rng.integers(0, TW, 12),
                     rng.integers(0, TH, 12)], axis=1).astype(np.int32)
    segs[4] = (0, TW, 0, 0, 0)  # out of range
    return E.ro(disp), xyz, E.ro(segs), RR.measure_xyz(xyz[0][None], segs)


def host_pair(inputs):
    """sdr_reproject with handle_missing 0 and 1 and sdr_measure_xyz on the calling thread, checked
    against the references."""
    disp, xyz, segs, recs = inputs
    for hm in (0, 1):
        out = np.full((TH, TW, 3), -777.25, np.float32)
        check(lib().sdr_reproject(disp.ctypes.data, TW, TH, TW, qptr(), hm, out.ctypes.data, 3 * TW))
        assert np.array_equal(out.view(np.uint32), xyz[hm].view(np.uint32)), f"sdr_reproject, handle_missing {hm}"
    rec = np.zeros(len(segs), MEASUREMENT_DTYPE)
    check(lib().sdr_measure_xyz(xyz[0].ctypes.data, TW * 3, TW * TH * 3, TW, TH, 1, segs.ctypes.data, len(segs),
                                rec.ctypes.data))
    RR.assert_records_equal(rec, recs)
    assert rec["flags"][4] == RR.OUT_OF_RANGE


class Worker(threading.Thread):
    """A thread that runs what it is handed, one task at a time, until it is handed None."""

    def __init__(self):
        super().__init__(daemon=True)
        self.tasks, self.done = queue.Queue(), queue.Queue()
        self.start()

    def run(self):
        for task in iter(self.tasks.get, None):
            try:
                task()
                self.done.put(None)
            except BaseException as e:  # noqa: BLE001 -- handed to the test's thread
                self.done.put(e)

    def call(self, task):
        self.tasks.put(task)
        err = self.done.get()
        if err is not None:
            raise err

    def exit(self):
        self.tasks.put(None)
        self.join()


def test_two_threads_alternating(thread_inputs):
    a, b = Worker(), Worker()
    try:
        for _ in range(3):
            a.call(lambda: host_pair(thread_inputs))
            b.call(lambda: host_pair(thread_inputs))
        b.exit()  # its state (stream, buffers, staging) is released with the thread
        assert not b.is_alive()
        a.call(lambda: host_pair(thread_inputs))
    finally:
        a.exit()
        b.exit()


def test_state_follows_the_current_device(thread_inputs):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")

    def task():
        try:
            host_pair(thread_inputs)
            torch.cuda.set_device(1)
            host_pair(thread_inputs)  # released on device 0, rebuilt on device 1
            torch.cuda.set_device(0)
            host_pair(thread_inputs)
        finally:
            torch.cuda.set_device(0)

    w = Worker()
    try:
        w.call(task)
    finally:
        w.exit()


# ---- the voxel grid over its planned arena ------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 257, 4097])  # one point; past a block; kRsTile + 1: a second sort tile
def test_voxel_grid_bit_exact(oracle, n):
    cid = f"size-{n}"
    pts, leaf = E.voxel_case(cid)
    ref, passthrough = E.voxel_reference(oracle, cid)
    assert len(pts) == n and not passthrough
    d_in = dev(pts)
    out = torch.full((n * 16 + 64,), E.SENT, dtype=torch.uint8, device="cuda")
    cnt, pt = ctypes.c_int(-7), ctypes.c_int(-7)
    check(lib().sdr_voxel_grid_device(d_in.data_ptr(), n, *leaf, out.data_ptr(), ctypes.byref(cnt), ctypes.byref(pt),
                                      _cstream(0)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert pt.value == 0 and cnt.value == len(ref)
    assert (got[n * 16:] == E.SENT).all(), "wrote past the output's capacity"
    assert np.array_equal(got[:cnt.value * 16].view(np.uint32).reshape(-1, 4), E.u32(ref))
