"""The point-cloud entry points (sdr_cloud.hip) at their sort, size and stride edges, BIT FOR BIT
against oracle/pcl_oracle.c on the clouds of emit_cases.py: voxel grids whose division product sits
on and next to 2^8, 2^16 and 2^24 (one to four passes of the radix sort, with the non-finite points'
marker on a digit boundary), point counts on and next to a block, a scan segment and a sort tile,
one finite point, none, no point at all, every permutation of an anisotropic leaf, cell indices past
2^24, voxels of 70 000 and 20 000 points (sums that depend on their order), PCL's passthrough
decision on either side of 2^31, identical points and points on cell boundaries; the organised cloud
with padded, sentinel-filled BGR rows and frames, without colour, and at the size where the
grid-stride loop takes a second trip; and the refusals.  test_emit_cases_cpu.py proves, without a
GPU, that the clouds have these properties."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import emit_cases as E  # noqa: E402
from stereo_depth_ruler_amd._lib import lib  # noqa: E402
from stereo_depth_ruler_amd.cloud import PointCloud, VoxelGrid  # noqa: E402
from stereo_depth_ruler_amd.sgbm import _cstream  # noqa: E402

ERR_ARG = -1
SENT = E.SENT
TAIL = 64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def sentinel(n):
    return torch.full((n,), SENT, dtype=torch.uint8, device="cuda")


def last_error():
    return lib().sdr_last_error().decode(errors="replace")


def voxel_raw(pts, leaf, n=None, expect=0):
    """sdr_voxel_grid_device through the raw ABI -> (points, passthrough); the output is a
    sentinel-filled buffer of n records and TAIL bytes, the count and the flag start at -7."""
    n = len(pts) if n is None else n
    d_in = dev(pts) if len(pts) else torch.zeros(4, dtype=torch.float32, device="cuda")
    cap = max(n, 0) * 16
    out = sentinel(cap + TAIL)
    cnt, pt = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib().sdr_voxel_grid_device(d_in.data_ptr(), n, *leaf, out.data_ptr(), ctypes.byref(cnt),
                                     ctypes.byref(pt), _cstream(0))
    torch.cuda.synchronize()
    assert rc == expect, (rc, last_error())
    got = out.cpu().numpy()
    assert (got[cap:] == SENT).all(), "wrote past the output's capacity"
    if rc:
        assert (got == SENT).all() and cnt.value == -7 and pt.value == -7, "a refused call wrote"
        assert last_error()
        return None, None
    assert 0 <= cnt.value <= n and pt.value in (0, 1)
    return got[:cnt.value * 16].view(np.float32).reshape(-1, 4), bool(pt.value)


@pytest.mark.parametrize("cid", E.VOXEL_IDS)
def test_voxel_case_bit_exact(oracle, cid):
    pts, leaf = E.voxel_case(cid)
    ref, passthrough = E.voxel_reference(oracle, cid)
    got, pt = voxel_raw(pts, leaf)
    assert pt == passthrough and got.shape == ref.shape
    assert np.array_equal(E.u32(got), E.u32(ref))


def test_voxel_no_points():
    got, pt = voxel_raw(np.empty((0, 4), np.float32), E.LEAF)
    assert got.shape == (0, 4) and not pt


def test_voxel_passthrough_keeps_the_organised_shape(oracle):
    """4097 = 17 x 241: past 2^31 the output is the input, shape included; just below it is a
    filtered, unorganised cloud."""
    vg = VoxelGrid()
    vg.setLeafSize(1.0, 1.0, 1.0)
    past, _ = E.voxel_case("edge-past")
    out = vg.filter(PointCloud(dev(past), 241, 17))
    assert vg.passthrough and (out.width, out.height) == (241, 17)
    assert np.array_equal(E.u32(out.points.cpu().numpy()), E.u32(past))
    below, _ = E.voxel_case("edge-below")
    out = vg.filter(PointCloud(dev(below), 241, 17))
    ref, _ = E.voxel_reference(oracle, "edge-below")
    assert not vg.passthrough and (out.width, out.height) == (len(ref), 1)
    assert np.array_equal(E.u32(out.points.cpu().numpy()), E.u32(ref))


def test_voxel_sizes_in_turn_on_one_arena(oracle):
    """The size cases largest first and then upwards again: the scratch arena is reused at every
    size below its capacity, with the previous call's keys and histograms still in it."""
    ids = [f"size-{n}" for n in E.SIZES[::-1] + E.SIZES] + ["none-finite", "band-256x256x256", "size-1"]
    for cid in ids:
        pts, leaf = E.voxel_case(cid)
        ref, passthrough = E.voxel_reference(oracle, cid)
        got, pt = voxel_raw(pts, leaf)
        assert pt == passthrough and np.array_equal(E.u32(got), E.u32(ref)), cid


def test_voxel_refusals():
    pts, leaf = E.voxel_case("size-257")
    voxel_raw(pts, leaf, n=-1, expect=ERR_ARG)
    for axis in range(3):
        for bad in (0.0, -0.5, float("nan"), -0.0):
            l = list(leaf)
            l[axis] = bad
            voxel_raw(pts, l, expect=ERR_ARG)
            assert "leaf" in last_error()
    d, out = dev(pts), sentinel(len(pts) * 16)
    cnt, pt = ctypes.c_int(-7), ctypes.c_int(-7)
    L = lib().sdr_voxel_grid_device
    assert L(None, len(pts), *leaf, out.data_ptr(), ctypes.byref(cnt), ctypes.byref(pt), _cstream(0)) == ERR_ARG
    assert "null" in last_error()
    assert L(d.data_ptr(), len(pts), *leaf, None, ctypes.byref(cnt), ctypes.byref(pt), _cstream(0)) == ERR_ARG
    assert L(d.data_ptr(), len(pts), *leaf, out.data_ptr(), None, ctypes.byref(pt), _cstream(0)) == ERR_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all() and cnt.value == -7 and pt.value == -7
    # the passthrough flag alone is optional
    assert L(d.data_ptr(), len(pts), *leaf, out.data_ptr(), ctypes.byref(cnt), None, _cstream(0)) == 0
    assert cnt.value > 0


# ---- sdr_xyz_to_cloud_device ----------------------------------------------------------------------

def cloud_raw(xyz, bgr, W, H, F, stride=0, fstride=0, expect=0, null=()):
    """The raw ABI on xyz (F, H, W, 3) and a BGR buffer laid out by the caller (or None)."""
    n = W * H * F
    d_xyz = dev(xyz)
    d_bgr = None if bgr is None else dev(bgr)
    out = sentinel(max(n, 0) * 16 + TAIL)
    rc = lib().sdr_xyz_to_cloud_device(None if "xyz" in null else d_xyz.data_ptr(),
                                       None if d_bgr is None else d_bgr.data_ptr(), stride, fstride, W, H, F,
                                       None if "out" in null else out.data_ptr(), _cstream(0))
    torch.cuda.synchronize()
    assert rc == expect, (rc, last_error())
    got = out.cpu().numpy()
    if rc:
        assert (got == SENT).all(), "a refused call wrote"
        assert last_error()
        return None
    assert (got[n * 16:] == SENT).all(), "wrote past the cloud's end"
    return got[:n * 16].view(np.float32).reshape(F, H * W, 4)


@pytest.mark.parametrize("shape", E.CLOUD_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_cloud_padded_frames_and_no_colour(oracle, shape):
    """Three frames (one at the size where the grid-stride loop takes its second trip: 8192 blocks of
    256 and one pixel more), BGR rows 5 bytes and frames 11 bytes longer than dense, the padding
    filled with a byte no pixel holds; dense strides passed as 0; and no colour at all."""
    W, H, F = shape
    xyz, bgr = E.cloud_frames(W, H, F)
    ref = np.stack([oracle.xyz_to_cloud(xyz[f], bgr[f]) for f in range(F)])
    stride = 3 * W + 5
    fstride = stride * H + 11
    buf = np.r_[E.padded_u8(bgr.reshape(F, H, 3 * W), stride, fstride), np.full(TAIL, SENT, np.uint8)]
    got = cloud_raw(xyz, buf, W, H, F, stride, fstride)
    assert np.array_equal(E.u32(got), E.u32(ref))
    colour = E.u32(got)[..., 3]
    for shift in (0, 8, 16):
        assert not ((colour >> shift) & 255 == SENT).any()
    # a padded row with frames dense at that row length (frame stride 0), and all dense (both 0)
    buf = np.r_[E.padded_u8(bgr.reshape(F, H, 3 * W), stride, stride * H), np.full(TAIL, SENT, np.uint8)]
    assert np.array_equal(E.u32(cloud_raw(xyz, buf, W, H, F, stride, 0)), E.u32(ref))
    assert np.array_equal(E.u32(cloud_raw(xyz, bgr.reshape(-1), W, H, F, 0, 0)), E.u32(ref))
    plain = np.stack([oracle.xyz_to_cloud(xyz[f], None) for f in range(F)])
    assert np.array_equal(E.u32(cloud_raw(xyz, None, W, H, F, 0, 0)), E.u32(plain))
    assert (E.u32(plain)[..., 3] == 0xFF000000).all()


def test_cloud_refusals():
    W, H, F = 37, 5, 3
    xyz, bgr = E.cloud_frames(W, H, F)
    flat = bgr.reshape(-1)
    for w, h, f in ((0, H, F), (-1, H, F), (W, 0, F), (W, -2, F), (W, H, 0), (W, H, -1)):
        cloud_raw(xyz, flat, w, h, f, expect=ERR_ARG)
        assert "size" in last_error()
    cloud_raw(xyz, flat, W, H, F, stride=3 * W - 1, fstride=3 * W * H, expect=ERR_ARG)
    assert "stride" in last_error()
    cloud_raw(xyz, flat, W, H, F, null=("xyz",), expect=ERR_ARG)
    cloud_raw(xyz, flat, W, H, F, null=("out",), expect=ERR_ARG)
    assert "null" in last_error()
