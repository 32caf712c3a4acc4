"""The mesh rasteriser on the MI355X (csrc/hl_mesh_raster.hip, humanliff_amd/NeRF/raster.py) against the numpy restatement
(tests/mesh_raster_restatement.py).  DESIGN.md "Rasterising the mesh".

Projection is tested once (case 1: device records against the float64 restatement); every later case feeds the device's OWN records
to the restatement, as tests/test_mesh_animate_gpu.py feeds it the device's rows, so those cases test coverage, depth and
interpolation, not projection again.  Coverage is exact integers: where no two surfaces compete, ids and acc must be equal at EVERY
pixel.  Where two surfaces compete the winner is decided by fp32 depths, so ids are compared where the float64 gap between the nearest
and the second-nearest depth is at least GAP = 1e-5 (depths are about 2: one fp32 ulp is 2.4e-7, a depth carries a few of them), and
the test asserts that at most 0.5 % of the doubly covered pixels are left out.  Values follow the rule of tests/test_body_gpu.py:
against the float64 restatement the kernel may be off by at most FACTOR = 4 x what the float32 restatement - the same formulas in the
kernel's stated order - is off by on the same inputs, per output.

Scenes: sheets of n x n jittered quads (numpy default_rng(seed), two triangles per quad), a pinhole camera with an off-centre
principal point, rotated 0.3 rad, T = (0.05, -0.02, 2.0), focal length 70; images are 67 x 48 unless stated."""
import numpy as np
import pytest
import torch

from tests import mesh_raster_restatement as mr

pytestmark = pytest.mark.gpu
FACTOR = 4.0
GAP = 1e-5
H, W = 48, 67
F32, F64 = np.float32, np.float64
VALUE_KEYS = ("depth_map", "barycentrics", "normal_map", "rgb_map")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


CAM = mr.scene_camera(H, W)


def attributes(N, seed):
    """Unit normals (one of them zero) and uint8 colours for N vertices."""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(N, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    n[N // 2] = 0.0
    return n, rng.integers(0, 256, (N, 3), dtype=np.uint8)


def merge(*meshes):
    vs, ts, o = [], [], 0
    for v, t in meshes:
        vs.append(v), ts.append(t + o)
        o += v.shape[0]
    return np.concatenate(vs).astype(F32), np.concatenate(ts).astype(np.int64)


def unproject(sx, sy, depth, cam=CAM):
    """The world point that projects to pixel coordinates (sx, sy) at camera z `depth` (float64)."""
    K, R, T = cam
    pc = np.linalg.inv(K) @ np.array([sx, sy, 1.0]) * depth
    return R.T @ (pc - T)


def box_mesh():
    """A 12-triangle box around the camera's view axis that fills the image and reaches beyond it; vertex 8 lies behind the camera and
    the last triangle uses it (that triangle is dropped: there is no near-plane clipping)."""
    c = [unproject(sx, sy, d) for d in (2.6, 3.4) for sy in (-30.0, H + 25.0) for sx in (-40.0, W + 35.0)]
    c.append(unproject(W / 2, H / 2, -0.5))
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tri = [t for a, b, c_, d in q for t in ((a, b, c_), (a, c_, d))]
    tri[-1] = (1, 8, 3)
    return np.array(c, F32), np.array(tri, np.int64)


def crossing(n):
    return merge(mr.sheet(n, seed=3, z0=0.0, amplitude=0.08), mr.sheet(n, seed=4, z0=0.02, amplitude=-0.08))


def rasterize(dev, v, tri, cam=CAM, h=H, w=W, **kw):
    """-> (outputs as numpy, device records int32 (F,N,4))."""
    from humanliff_amd.NeRF import raster
    out, scratch = raster._rasterize(v, tri, h, w, *cam, **kw)
    torch.cuda.synchronize()
    F = out["acc_map"].shape[0]
    recs = raster.scratch_records(scratch, np.asarray(v).shape[-2], F).cpu().numpy()
    return {k: t.cpu().numpy() for k, t in out.items()}, recs


def split(rec):
    """Records (N,4) of one image -> X, Y int64, z float32, invalid."""
    return rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64), rec[:, 2].copy().view(F32), (rec[:, 3] & 1) != 0


def restate(rec, v, tri, dtype, cam=CAM, h=H, w=W, normals=None, colors=None, shade="colors", white_bkgd=False, cull=None):
    X, Y, z, bad = split(rec)
    c = mr.cover(X, Y, z, tri, h, w, dtype=dtype, invalid=bad, cull=cull)
    r = mr.resolve(X, Y, z, tri, c["id"], c["depth"], v, *cam, normals=normals, colors=colors, shade=shade, white_bkgd=white_bkgd, dtype=dtype)
    r.update(id=c["id"], depth2=c["depth2"], hits=c["hits"])
    return r


_CACHE = {}


def case(dev, name, make, **kw):
    """One scene rasterised on the device and restated in float32 and float64 from the device's records, each once."""
    if name not in _CACHE:
        v, tri = make()
        n, col = attributes(v.shape[0], 11)
        out, recs = rasterize(dev, v, tri, normals=n, colors=col, **kw)
        r32, r64 = (restate(recs[0], v, tri, dt, normals=n, colors=col, **kw) for dt in (F32, F64))
        _CACHE[name] = dict(v=v, tri=tri, n=n, col=col, out=out, recs=recs, r32=r32, r64=r64)
    return _CACHE[name]


def settled(r64):
    """Pixels whose winner the float64 depths decide by at least GAP (background and singly covered pixels included)."""
    return ~((r64["hits"] >= 2) & (r64["depth2"] - r64["depth_map"] < GAP))


def check_ids(tag, s, cap=0.005):
    ok = settled(s["r64"])
    double = s["r64"]["hits"] >= 2
    left_out = int((~ok).sum())
    print(f"{tag}: {int(double.sum())} doubly covered pixels, {left_out} left out; min gap {np.min((s['r64']['depth2'] - s['r64']['depth_map'])[double], initial=np.inf):.2e}")
    assert left_out <= cap * max(int(double.sum()), 1)
    assert np.array_equal(s["out"]["triangle_id"][0][ok], s["r64"]["id"][ok])
    assert np.array_equal(s["out"]["acc_map"][0], (s["r64"]["id"] >= 0).astype(F32))
    return ok


def check_values(tag, s, keys=VALUE_KEYS, least=100):
    same = (s["out"]["triangle_id"][0] == s["r64"]["id"]) & (s["r32"]["id"] == s["r64"]["id"]) & (s["r64"]["id"] >= 0)
    assert same.sum() > least
    for k in keys:
        ek = float(np.abs(s["out"][k][0].astype(F64) - s["r64"][k])[same].max())
        ey = float(np.abs(s["r32"][k].astype(F64) - s["r64"][k])[same].max())
        print(f"{tag} {k}: kernel {ek:.3e}, fp32 restatement {ey:.3e}")
        assert ek <= FACTOR * ey, (tag, k, ek, ey)


# ---- 1. projection ------------------------------------------------------------------------------------------------------------
def test_projection(dev):
    v, tri = mr.sheet(8, seed=3)
    o = mr.camera_centre(CAM[1], CAM[2])
    extra = np.array([unproject(30.0, 20.0, -1.0), [np.nan, 0.0, 0.0], unproject(3e6, 20.0, 2.0), unproject(30.0, 20.0, 5e-4), o], F32)
    v = np.concatenate([v, extra]).astype(F32)
    _, recs = rasterize(dev, v, tri)
    X, Y, z, bad = split(recs[0])
    X64, Y64, z64, bad64 = mr.project(v, *CAM)
    assert bad64[-5:].all() and not bad64[:-5].any()
    assert np.array_equal(bad, bad64)
    good = ~bad64
    dx, dy = np.abs(X - X64)[good].max(), np.abs(Y - Y64)[good].max()
    print(f"projection: max |dX| {dx}, |dY| {dy} units of 1/256 pixel; {int((X != X64)[good].sum() + (Y != Y64)[good].sum())} coordinates differ")
    assert dx <= 1 and dy <= 1
    assert np.array_equal(z[good].view(np.uint32), z64[good].view(np.uint32))


# ---- 2. coverage --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 40])
def test_coverage_is_exact(dev, n):
    s = case(dev, f"sheet{n}", lambda: mr.sheet(n, seed=3))
    assert s["r64"]["hits"].max() == 1 and (s["r64"]["hits"] == 1).sum() > 900
    assert np.array_equal(s["out"]["triangle_id"][0], s["r64"]["id"])
    assert np.array_equal(s["out"]["acc_map"][0], (s["r64"]["id"] >= 0).astype(F32))
    check_values(f"sheet n={n}", s)


# ---- 3. depth resolution ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shade", [(8, "headlight"), (40, "colors")])
def test_depth_resolution(dev, n, shade):
    s = case(dev, f"crossing{n}", lambda: crossing(n), shade=shade)
    assert (s["r64"]["hits"] == 2).sum() > 800
    front = s["r64"]["id"][s["r64"]["hits"] == 2] < 2 * n * n
    assert 0.1 < front.mean() < 0.9                                              # the sheets do cross: each wins somewhere
    check_ids(f"crossing n={n}", s)
    check_values(f"crossing n={n} {shade}", s)
    hit = s["out"]["acc_map"][0] > 0
    assert np.array_equal(s["out"]["depth_map"][0][~hit], np.zeros((~hit).sum(), F32)) and (s["out"]["depth_map"][0][hit] > 0).all()


# ---- 4. the large path --------------------------------------------------------------------------------------------------------
def test_large_box(dev):
    s = case(dev, "box", box_mesh)
    X, Y, z, bad = split(s["recs"][0])
    assert bad[8] and not bad[:8].any()
    ok = check_ids("box", s)
    assert (s["out"]["triangle_id"][0] >= 0).all() and not (s["out"]["triangle_id"][0] == 11).any()      # fills the view; the dropped one
    assert len(np.unique(s["out"]["triangle_id"][0][ok])) >= 2
    check_values("box", s)


def test_large_box_behind_a_fine_sheet(dev):
    s = case(dev, "box+sheet", lambda: merge(box_mesh(), mr.sheet(40, seed=5)))
    ids = s["out"]["triangle_id"][0]
    assert (ids >= 12).sum() > 900 and ((ids >= 0) & (ids < 12)).sum() > 900
    check_ids("box + sheet", s)
    check_values("box + sheet", s)


def test_small_box_threshold(dev):
    """Two right triangles whose clamped boxes hold exactly small_box and small_box + 1 pixels: the last that a thread loops over
    itself and the first that goes to the list."""
    from humanliff_amd import _lib
    small = int(_lib.lib().hl_mesh_raster_small_box())
    assert small == 64
    v = np.array([unproject(10.6, 5.6, 2.0), unproject(18.4, 5.6, 2.1), unproject(10.6, 13.4, 1.9),          # columns 11..18, rows 6..13
                  unproject(30.6, 20.6, 2.0), unproject(35.4, 20.6, 2.1), unproject(30.6, 33.4, 1.9)], F32)   # columns 31..35, rows 21..33
    tri = np.array([[0, 1, 2], [3, 4, 5]], np.int64)
    out, recs = rasterize(dev, v, tri)
    X, Y, z, bad = split(recs[0])
    boxes = [((X[t].max() // 256) - (-(-X[t].min() // 256)) + 1) * ((Y[t].max() // 256) - (-(-Y[t].min() // 256)) + 1) for t in tri]
    assert boxes == [small, small + 1]
    r64 = restate(recs[0], v, tri, F64)
    assert np.array_equal(out["triangle_id"][0], r64["id"]) and (r64["id"] == 0).sum() > 20 and (r64["id"] == 1).sum() > 20
    r32 = restate(recs[0], v, tri, F32)
    check_values("threshold", dict(out=out, r32=r32, r64=r64), keys=("depth_map", "barycentrics"), least=40)


# ---- 5. order independence ----------------------------------------------------------------------------------------------------
def test_reproducible_and_order_independent(dev):
    s = case(dev, "crossing40", lambda: crossing(40), shade="colors")
    again, _ = rasterize(dev, s["v"], s["tri"], normals=s["n"], colors=s["col"])
    for k in s["out"]:
        assert np.array_equal(again[k].view(np.uint32), s["out"][k].view(np.uint32)), k
    perm = np.random.default_rng(9).permutation(s["tri"].shape[0])
    shuffled, _ = rasterize(dev, s["v"], s["tri"][perm], normals=s["n"], colors=s["col"])
    for k in ("depth_map", "acc_map"):
        assert np.array_equal(shuffled[k].view(np.uint32), s["out"][k].view(np.uint32)), k
    ok = settled(s["r64"]) & (s["out"]["triangle_id"][0] >= 0)
    assert np.array_equal(perm[shuffled["triangle_id"][0][ok]], s["out"]["triangle_id"][0][ok])
    assert np.array_equal(shuffled["triangle_id"][0] < 0, s["out"]["triangle_id"][0] < 0)
    # the box goes through the list, whose order depends on scheduling: the same bits all the same
    b = case(dev, "box+sheet", lambda: merge(box_mesh(), mr.sheet(40, seed=5)))
    again, _ = rasterize(dev, b["v"], b["tri"], normals=b["n"], colors=b["col"])
    for k in b["out"]:
        assert np.array_equal(again[k].view(np.uint32), b["out"][k].view(np.uint32)), k


# ---- 6. batching --------------------------------------------------------------------------------------------------------------
def _cameras3():
    K, R, T = CAM
    Ks = np.stack([K, K + np.array([[3.0, 0, 1.5], [0, 3.0, -2.0], [0, 0, 0]]), K])
    c, s_ = np.cos(0.2), np.sin(0.2)
    Ry = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
    return Ks, np.stack([R, R @ Ry, R @ Ry.T]), np.stack([T, T + [0.02, 0.0, 0.1], T + [-0.03, 0.01, -0.1]])


@pytest.mark.parametrize("layout", ["F3C3", "F3C1", "F1C3"])
def test_batching(dev, layout):
    v0, tri = merge(box_mesh(), mr.sheet(12, seed=5))
    n0, col = attributes(v0.shape[0], 11)
    rng = np.random.default_rng(21)
    nF, nC = int(layout[1]), int(layout[3])
    v = np.stack([v0] + [v0 + rng.normal(0, 0.01, v0.shape).astype(F32) for _ in range(nF - 1)])
    n = np.stack([n0] + [np.roll(n0, k + 1, axis=0) for k in range(nF - 1)])
    Ks, Rs, Ts = _cameras3()
    cam = (Ks, Rs, Ts) if nC == 3 else CAM
    batch, _ = rasterize(dev, v if nF == 3 else v[0], tri, cam=cam, normals=n if nF == 3 else n[0], colors=col, shade="headlight")
    assert batch["rgb_map"].shape == (3, H, W, 3)
    for i in range(3):
        one_cam = (Ks[i], Rs[i], Ts[i]) if nC == 3 else CAM
        one, _ = rasterize(dev, v[i if nF == 3 else 0], tri, cam=one_cam, normals=n[i if nF == 3 else 0], colors=col, shade="headlight")
        for k in batch:
            assert np.array_equal(batch[k][i].view(np.uint32), one[k][0].view(np.uint32)), (layout, i, k)
    assert not np.array_equal(batch["depth_map"][0], batch["depth_map"][1])


# ---- 7. convention ------------------------------------------------------------------------------------------------------------
def test_depth_is_the_ray_parameter(dev):
    """rays_o + depth_map * rays_d of camera_rays (same K, R, T) lies on the plane of the winning triangle."""
    from humanliff_amd.SynBodyView_datasets import camera_rays
    s = case(dev, "crossing40", lambda: crossing(40), shade="colors")
    ro, rd = (t.cpu().numpy().astype(F64).reshape(H, W, 3) for t in camera_rays(H, W, *CAM, np.array([[-1.0, -1, -1], [1, 1, 1]]), dev)[:2])
    same = (s["out"]["triangle_id"][0] == s["r64"]["id"]) & (s["r32"]["id"] == s["r64"]["id"]) & (s["r64"]["id"] >= 0)
    t = s["tri"][s["r64"]["id"][same]]
    v = s["v"].astype(F64)
    nrm = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)

    def off_plane(depth):
        p = ro[same] + depth[same].astype(F64)[:, None] * rd[same]
        return float((np.abs(((p - v[t[:, 0]]) * nrm).sum(axis=1)) / depth[same]).max())
    ek, ey = off_plane(s["out"]["depth_map"][0]), off_plane(s["r32"]["depth_map"])
    print(f"distance from the winning triangle's plane over depth: kernel {ek:.3e}, fp32 restatement {ey:.3e}")
    assert ek <= FACTOR * ey and ek < 1e-3


def test_pixel_centres_are_integers(dev):
    """A camera-facing quad whose corners project exactly onto the pixel centres (10,8) and (20,16): its top and left edges are
    owned, its right and bottom edges are not."""
    K = np.array([[64.0, 0, 32.0], [0, 64.0, 24.0], [0, 0, 1.0]])
    cam = (K, np.eye(3), np.zeros(3))
    c = lambda px, py: [(px - 32.0) / 64.0 * 2.0, (py - 24.0) / 64.0 * 2.0, 2.0]  # noqa: E731
    v = np.array([c(10, 8), c(20, 8), c(20, 16), c(10, 16)], F32)
    for tri in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 3, 2]], [[1, 2, 3], [1, 3, 0]]):
        out, recs = rasterize(dev, v, np.array(tri, np.int64), cam=cam)
        assert np.array_equal(recs[0][:, :2], np.array([[10, 8], [20, 8], [20, 16], [10, 16]]) * 256)
        want = np.zeros((H, W), F32)
        want[8:16, 10:20] = 1.0
        assert np.array_equal(out["acc_map"][0], want)
        assert np.array_equal(out["depth_map"][0], want * 2.0)


# ---- 8. attributes and options ------------------------------------------------------------------------------------------------
def test_options(dev):
    s = case(dev, "crossing8", lambda: crossing(8), shade="headlight")
    v, tri, n, col, rec = s["v"], s["tri"], s["n"], s["col"], s["recs"][0]
    hit = s["r64"]["id"] >= 0
    # without normals: flat, unit, facing the camera
    out, _ = rasterize(dev, v, tri, colors=col, white_bkgd=True)
    st = dict(out=out, r32=restate(rec, v, tri, F32, colors=col, white_bkgd=True), r64=restate(rec, v, tri, F64, colors=col, white_bkgd=True))
    check_values("flat normals", st)
    rays = mr.ray_directions(H, W, *CAM)
    assert ((out["normal_map"][0].astype(F64) * rays).sum(axis=-1)[hit] < 0).all()
    assert np.abs(np.linalg.norm(out["normal_map"][0][hit].astype(F64), axis=-1) - 1).max() < 1e-6
    assert (out["rgb_map"][0][~hit] == 1).all() and (out["normal_map"][0][~hit] == 0).all() and (out["barycentrics"][0][~hit] == 0).all()
    assert (out["triangle_id"][0][~hit] == -1).all()
    # without colours: grey; times the headlight term
    out, _ = rasterize(dev, v, tri, normals=n)
    assert (out["rgb_map"][0][hit] == F32(0.7)).all() and (out["rgb_map"][0][~hit] == 0).all()
    out, _ = rasterize(dev, v, tri, normals=n, shade="headlight")
    st = dict(out=out, r32=restate(rec, v, tri, F32, normals=n, shade="headlight"), r64=restate(rec, v, tri, F64, normals=n, shade="headlight"))
    check_values("grey headlight", st, keys=("rgb_map",))
    # the vertex with the zero normal: the interpolated normal is unit or zero, never NaN
    assert np.isfinite(s["out"]["normal_map"]).all()
    # culling: exactly the triangles of negative A go
    X, Y, z, bad = split(rec)
    flipped = tri.copy()
    flipped[::3] = flipped[::3][:, [0, 2, 1]]
    for cull in ("back", "front"):
        out, _ = rasterize(dev, v, flipped, normals=n, colors=col, cull=cull)
        keep = mr.drawn(X, Y, bad, flipped, cull=cull)
        assert 0 < keep.sum() < keep.size
        r64 = restate(rec, v, flipped, F64, normals=n, colors=col, cull=cull)
        ok = settled(r64)
        assert np.array_equal(out["triangle_id"][0][ok], r64["id"][ok]) and keep[out["triangle_id"][0][out["triangle_id"][0] >= 0]].all()
        assert np.array_equal(out["acc_map"][0], (r64["id"] >= 0).astype(F32))


def test_degenerate_and_out_of_range_triangles(dev):
    v, tri = mr.sheet(8, seed=3)
    N = v.shape[0]
    base, _ = rasterize(dev, v, tri)
    extra = np.array([[0, 0, 5], [3, 3, 3], [0, 1, N], [-1, 2, 3], [2, 1 << 40, 3]], np.int64)      # two degenerate, three out of range
    both = np.concatenate([tri, extra])
    from humanliff_amd.NeRF import raster
    with pytest.raises(ValueError, match="outside"):
        raster.rasterize(v, both, H, W, *CAM)
    out, _ = rasterize(dev, v, both, check_indices=False)
    for k in base:
        assert np.array_equal(out[k].view(np.uint32), base[k].view(np.uint32)), k
    out, _ = rasterize(dev, v, both[:-3])                                        # degenerate ones alone raise nothing
    assert np.array_equal(out["triangle_id"], base["triangle_id"])
    # the library refuses empty sizes with its error code
    from humanliff_amd import _lib
    L = _lib.lib()
    assert L.hl_mesh_raster_scratch_bytes(0, 5, 1, H, W) == 0 and L.hl_mesh_raster_scratch_bytes(5, 0, 1, H, W) == 0
    assert L.hl_mesh_raster_scratch_bytes(5, 5, 1, 0, W) == 0 and L.hl_mesh_raster_scratch_bytes(5, 5, 0, H, W) == 0
    t = torch.zeros(64, device=dev)
    table = np.zeros(30)
    for Nn, Tt, Hh in ((0, 5, H), (5, 0, H), (5, 5, 0)):
        rc = L.hl_mesh_raster(_lib.ptr(t), 1, Nn, _lib.ptr(t.int(), torch.int32), Tt, None, 0, None, table.ctypes.data, 0, 1, Hh, W, 1e-3, 0,
                              _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), None, None, None, _lib.ptr(t), 256, _lib.stream_ptr(dev))
        assert rc != 0 and b"bad sizes" in L.hl_last_error()


def test_guards_stay_untouched(dev):
    """Sentinels around every output and around the scratch, which is exactly as long as the query says: the outputs and the scratch
    are carved out of buffers with 64 sentinel elements on either side (the same bits whether a buffer holds int32 or, rounded, fp32)."""
    from humanliff_amd import _lib
    from humanliff_amd.NeRF import raster
    v, tri = merge(box_mesh(), mr.sheet(12, seed=5))
    n, col = attributes(v.shape[0], 11)
    Ks, Rs, Ts = _cameras3()
    guard, sentinel, guards, sizes = 64, 0x5A5A5A5A, [], []

    def alloc(shape, dtype):
        size = int(np.prod(shape))
        buf = torch.full((size + 2 * guard,), sentinel, dtype=dtype, device=dev)
        guards.append((buf[:guard], buf[guard + size:]))
        sizes.append(size)
        return buf[guard:guard + size].view(shape)
    out, scratch = raster._rasterize(v, tri, H, W, Ks, Rs, Ts, normals=n, colors=col, shade="headlight", alloc=alloc)
    torch.cuda.synchronize()
    assert len(guards) == 7 and scratch.dtype == torch.int32
    assert sizes[-1] * 4 == scratch.numel() * 4 == _lib.lib().hl_mesh_raster_scratch_bytes(v.shape[0], tri.shape[0], 3, H, W)
    for lo, hi in guards:
        assert lo.numel() == guard and hi.numel() == guard and bool((lo == sentinel).all()) and bool((hi == sentinel).all())
    plain, _ = rasterize(dev, v, tri, cam=(Ks, Rs, Ts), normals=n, colors=col, shade="headlight")
    for k in plain:
        assert np.array_equal(out[k].cpu().numpy().view(np.uint32), plain[k].view(np.uint32)), k


# ---- 9. through the pipeline --------------------------------------------------------------------------------------------------
def test_binding_rasterize(dev):
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import animate, raster
    from humanliff_amd.body import load_body_model
    model = load_body_model(syn.smpl_like_model(1200, 3), dev)
    g = syn._gen(77)
    poses = (torch.randn((3, 72), generator=g) * 0.25).to(dev)
    posed = model.pose(poses, torch.zeros(10, device=dev), forward_rows=True)
    body = posed.vertices[0].cpu().numpy().astype(F64)
    centre = body.mean(axis=0)
    sv, tri = mr.sheet(12, seed=6, extent=0.6)
    sv = (sv.astype(F64) + centre + [0, 0, 0.15]).astype(F32)
    n, col = attributes(sv.shape[0], 5)
    binding = animate.bind_mesh(sv, posed, frame=0, neighbours=4, normals=n)
    binding.triangles, binding.colors = tri, col
    K = np.array([[40.0, 0, W / 2.0], [0, 40.0, H / 2.0], [0, 0, 1.0]])
    cam = (K, np.eye(3), np.array([0.0, 0.0, 2.2]) - centre)
    got = binding.rasterize(posed, H, W, *cam, shade="headlight")
    moved = binding.repose(posed, bounds=False)
    want = raster.rasterize(moved["vertices"], tri, H, W, *cam, normals=moved["normals"], colors=col, shade="headlight")
    assert got["rgb_map"].shape == (3, H, W, 3) and float(got["acc_map"].sum()) > 300
    for k in want:
        assert torch.equal(got[k], want[k]), k
    one = binding.rasterize(posed, H, W, *cam, frames=1, shade="headlight")
    for k in want:
        assert torch.equal(one[k][0], want[k][1]), k
