"""Mesh extraction on the device: PyMCubes' `smooth` (constrained branch) and `marching_cubes` on HIP (hl_geometry.hip).

The reference meshes a density lattice with mcubes.marching_cubes(mcubes.smooth(u), threshold) (NeRF/renderer.py:290-321,
recon_NeRF/lib/renderer.py:304-348); Renderer.extract_geometry(..., mesher="hip") runs the same two steps through this module.
The contract - signed distance, band, bounds, operator, stopping rule, corner rule, case table and ordering - is DESIGN.md
"Mesh extraction".  CPU tensors raise: there is no host fallback.
"""
import numpy as np
import torch

from .. import _lib

W_STOP_EVERY = 10     # energy check period of the Jacobi loop


class NoSignChange(ValueError):
    """The volume lies on one side of 0: there is no surface to smooth or mesh."""


def _volume(volume, dtypes, what):
    if not isinstance(volume, torch.Tensor) or not volume.is_cuda:
        raise RuntimeError(f"{what} needs a device tensor (no CPU path)")
    if volume.dim() != 3:
        raise ValueError(f"{what}: expected a 3-D volume, got shape {tuple(volume.shape)}")
    if volume.dtype not in dtypes:
        raise TypeError(f"{what}: volume must be one of {dtypes}, got {volume.dtype}")
    return volume.contiguous()


def _ws(nbytes, what, device):
    if nbytes == 0:
        raise ValueError(f"{what}: volume outside the supported sizes (nx*ny*nz*5 < 2^31)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def smooth_constrained(volume, band_radius=4, max_iters=250, rel_tol=1e-6, return_info=False):
    """mcubes.smooth_constrained with its defaults: fp64 device volume - the signed distance of `volume > 0` outside the band
    |d| <= band_radius, the constrained minimiser of the squared Laplacian energy inside it.  ValueError if the volume has no sign
    change.  return_info=True also returns (sweeps run, band size)."""
    v = _volume(volume, (torch.float32, torch.float64), "smooth_constrained")
    L = _lib.lib()
    dev = v.device
    nx, ny, nz = (int(s) for s in v.shape)
    with _lib.on(dev):
        st = _lib.stream_ptr(dev)
        ws = _ws(L.hl_smooth_workspace_bytes(nx, ny, nz), "smooth_constrained", dev)
        out = torch.empty((nx, ny, nz), dtype=torch.float64, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        _lib.check(L.hl_smooth_prepare(_dptr(v), int(v.dtype == torch.float64), nx, ny, nz, float(band_radius), _dptr(out),
                                       _lib.ptr(counts), _dptr(ws), ws.numel(), st), "hl_smooth_prepare")
        nb, n_pos = (int(c) for c in counts.cpu())
        if n_pos == 0 or n_pos == nx * ny * nz:
            raise NoSignChange("smooth_constrained: the volume has no sign change (all voxels on one side of 0)")
        lin = torch.empty(nb, dtype=torch.int32, device=dev)
        nbr = torch.empty((6, nb), dtype=torch.int32, device=dev)
        x, lower, upper = (torch.empty(nb, dtype=torch.float64, device=dev) for _ in range(3))
        _lib.check(L.hl_smooth_band(_dptr(out), nx, ny, nz, float(band_radius), nb, _lib.ptr(lin, torch.int32), _lib.ptr(nbr, torch.int32),
                                    _dptr(x), _dptr(lower), _dptr(upper), _dptr(ws), ws.numel(), st), "hl_smooth_band")
        del ws
        scr = _ws(L.hl_smooth_sweep_scratch_bytes(nb), "smooth_constrained", dev)
        energy = torch.zeros(1, dtype=torch.float64, device=dev)

        def sweeps(k, with_energy):
            _lib.check(L.hl_smooth_sweeps(_lib.ptr(nbr, torch.int32), _dptr(lower), _dptr(upper), nb, k, _dptr(x),
                                          _dptr(energy) if with_energy else None, _dptr(scr), scr.numel(), st), "hl_smooth_sweeps")

        sweeps(0, True)
        e_prev = float(energy.cpu())
        it = 0
        stop = 1 - (1 - rel_tol) ** W_STOP_EVERY
        while it < max_iters:
            k = min(W_STOP_EVERY, max_iters - it)
            check = (it + k) % W_STOP_EVERY == 0
            sweeps(k, check)
            it += k
            if check:
                e = float(energy.cpu())
                ratio = (e_prev - e) / e_prev if e_prev != 0 else float("nan")
                if ratio < stop:          # (NaN never stops)
                    break
                e_prev = e
        _lib.check(L.hl_smooth_scatter(_dptr(x), _lib.ptr(lin, torch.int32), nb, _dptr(out), st), "hl_smooth_scatter")
    return (out, (it, nb)) if return_info else out


def smooth(volume, method="auto"):
    """mcubes.smooth: `auto` takes the constrained branch up to 512^3 voxels (as PyMCubes does); the Gaussian branch PyMCubes
    takes above that is not implemented."""
    if method == "auto":
        if volume.numel() > 512 ** 3:
            raise NotImplementedError("smooth: volumes above 512^3 take PyMCubes' Gaussian branch, which is not implemented")
        method = "constrained"
    if method != "constrained":
        raise NotImplementedError(f"smooth: method {method!r} is not implemented (constrained only)")
    return smooth_constrained(volume)


def marching_cubes(volume, isovalue):
    """mcubes.marching_cubes on a device fp64 volume: (vertices float64 (V,3) in index coordinates, triangles int64 (T,3)), both on
    the device.  One vertex per crossing lattice edge, ordered by edge key; triangles by cube, normals toward values > isovalue."""
    v = _volume(volume, (torch.float64,), "marching_cubes")
    L = _lib.lib()
    dev = v.device
    nx, ny, nz = (int(s) for s in v.shape)
    with _lib.on(dev):
        st = _lib.stream_ptr(dev)
        ws = _ws(L.hl_mc_workspace_bytes(nx, ny, nz), "marching_cubes", dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        _lib.check(L.hl_mc_count(_dptr(v), nx, ny, nz, float(isovalue), _lib.ptr(counts), _dptr(ws), ws.numel(), st), "hl_mc_count")
        nv, nt = (int(c) for c in counts.cpu())
        verts = torch.empty((nv, 3), dtype=torch.float64, device=dev)
        tris = torch.empty((nt, 3), dtype=torch.int64, device=dev)
        _lib.check(L.hl_mc_emit(_dptr(v), nx, ny, nz, float(isovalue), _dptr(verts), _lib.ptr(tris), _dptr(ws), ws.numel(), st),
                   "hl_mc_emit")
    return verts, tris


def case_table():
    """The baked marching-cubes table: list over the 256 corner configurations of [(e0, e1, e2), ...] cube edges."""
    import ctypes as C
    L = _lib.lib()
    mt = L.hl_mc_max_triangles()
    tris = np.zeros((256, mt, 3), dtype=np.int8)
    ntri = np.zeros(256, dtype=np.uint8)
    _lib.check(L.hl_mc_case_table(tris.ctypes.data_as(C.c_void_p), ntri.ctypes.data_as(C.c_void_p)), "hl_mc_case_table")
    return [[tuple(int(e) for e in tris[c, t]) for t in range(ntri[c])] for c in range(256)]


def write_ply(path, vertices, triangles):
    """Binary little-endian PLY: float64 vertices, one (uchar 3, int32 x3) list per face.  The reference writes its meshes with
    trimesh, which this package does not depend on; any PLY reader loads this."""
    v = np.ascontiguousarray(np.asarray(vertices.cpu() if isinstance(vertices, torch.Tensor) else vertices, dtype="<f8").reshape(-1, 3))
    t = np.asarray(triangles.cpu() if isinstance(triangles, torch.Tensor) else triangles).reshape(-1, 3)
    if len(v) and t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("write_ply: triangle index out of range")
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {len(v)}\nproperty double x\nproperty double y\nproperty double z\n"
            f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    face = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    face["n"] = 3
    face["i"] = t
    with open(path, "wb") as f:
        f.write(head)
        f.write(v.tobytes())
        f.write(face.tobytes())


def read_ply(path):
    """Reads back what write_ply wrote: (vertices float64 (V,3), triangles int64 (T,3))."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nt = int(next(h for h in head if h.startswith("element face")).split()[-1])
    v = np.frombuffer(data, dtype="<f8", count=nv * 3, offset=end).reshape(nv, 3)
    face = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nt, offset=end + nv * 24)
    assert (face["n"] == 3).all()
    return v.copy(), face["i"].astype(np.int64)


def _dptr(t):
    """Device pointer of an fp64 / fp32 / byte tensor (the ABI's double* and void* arguments)."""
    return _lib.ptr(t, dtype=t.dtype)
