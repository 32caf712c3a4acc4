"""Mesh extraction on the device: PyMCubes' `smooth` (constrained branch) and `marching_cubes` on HIP (hl_geometry.hip).

The reference meshes a density lattice with mcubes.marching_cubes(mcubes.smooth(u), threshold) (NeRF/renderer.py:290-321,
recon_NeRF/lib/renderer.py:304-348); Renderer.extract_geometry(..., mesher="hip") runs the same two steps through this module.
The contract - signed distance, band, bounds, operator, stopping rule, corner rule, case table and ordering - is DESIGN.md
"Mesh extraction".  Beside the reference: the connected components of the solid side, the component filter and the vertex normals
behind Renderer.extract_mesh ("Finishing the mesh" there).  CPU tensors raise: there is no host fallback.
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


def vertex_normals(volume, isovalue, vertices_index_coords, extent=None):
    """Unit normals fp64 (V,3) of marching_cubes(volume, isovalue)'s vertices, in their order: the field's central-difference gradient
    (one-sided at a volume face) interpolated along each vertex's lattice edge, divided per axis by `extent` (the world extent of the
    lattice, default 1) and normalised.  +gradient points to the above side, so the normals point out of the body; a zero vector stays
    zero.  The edges are taken from the volume's edge keys, not from the positions: `vertices_index_coords` must be that call's
    vertices, and only its count is checked."""
    v = _volume(volume, (torch.float64,), "vertex_normals")
    L = _lib.lib()
    dev = v.device
    nx, ny, nz = (int(s) for s in v.shape)
    nv = int(vertices_index_coords.shape[0])
    if tuple(vertices_index_coords.shape) != (nv, 3):
        raise ValueError(f"vertex_normals: vertices must be (V,3), got {tuple(vertices_index_coords.shape)}")
    ext = None
    if extent is not None:
        ext = np.ascontiguousarray((extent.detach().cpu() if isinstance(extent, torch.Tensor) else extent), dtype=np.float64).reshape(3)
    with _lib.on(dev):
        st = _lib.stream_ptr(dev)
        ws = _ws(L.hl_mc_workspace_bytes(nx, ny, nz), "vertex_normals", dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        _lib.check(L.hl_mc_count(_dptr(v), nx, ny, nz, float(isovalue), _lib.ptr(counts), _dptr(ws), ws.numel(), st), "hl_mc_count")
        have = int(counts[0].cpu())
        if have != nv:
            raise ValueError(f"vertex_normals: {nv} vertices given, the volume has {have} at this isovalue")
        normals = torch.empty((nv, 3), dtype=torch.float64, device=dev)
        keys = torch.empty(nv, dtype=torch.int32, device=dev)
        _lib.check(L.hl_mc_vertex_normals(_dptr(v), nx, ny, nz, float(isovalue), ext.ctypes.data if ext is not None else None, nv,
                                          _dptr(keys), _dptr(normals), _dptr(ws), ws.numel(), st), "hl_mc_vertex_normals")
    return normals


def label_components(volume, isovalue):
    """26-connected components of the solid side `!(volume > isovalue)` of a device fp64 volume: (labels int32 (nx,ny,nz), sizes int64
    (n,)).  Labels are 0 off the solid side and 1..n on it, numbered by the smallest C-order index of each component (the numbering
    of scipy.ndimage.label with the full 3x3x3 structure); sizes[i] is the voxel count of label i+1."""
    labels, sizes, _ = _label_components(volume, isovalue)
    return labels, sizes


def _label_components(volume, isovalue):
    """label_components plus the number of link / flatten rounds the labelling ran."""
    v = _volume(volume, (torch.float64,), "label_components")
    L = _lib.lib()
    dev = v.device
    nx, ny, nz = (int(s) for s in v.shape)
    with _lib.on(dev):
        st = _lib.stream_ptr(dev)
        ws = _ws(L.hl_cc_workspace_bytes(nx, ny, nz), "label_components", dev)
        labels = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        _lib.check(L.hl_cc_label(_dptr(v), nx, ny, nz, float(isovalue), _dptr(labels), _lib.ptr(counts), _dptr(ws), ws.numel(), st),
                   "hl_cc_label")
        n, rounds = (int(c) for c in counts.cpu())
        sizes = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.check(L.hl_cc_sizes(_dptr(labels), nx * ny * nz, n, _lib.ptr(sizes) if n else None, st), "hl_cc_sizes")
    return labels, sizes, rounds


def select_components(sizes, keep):
    """The labels (int64, ascending) that `keep` selects from `sizes`: "largest", an int k (the k largest; all when k exceeds their
    number) or ("min_voxels", m).  Ties in size go to the lower label."""
    n = int(sizes.numel())
    if isinstance(keep, (tuple, list)):
        if len(keep) != 2 or keep[0] != "min_voxels":
            raise ValueError(f"keep_components: keep must be 'largest', an int or ('min_voxels', m), got {keep!r}")
        return torch.nonzero(sizes >= int(keep[1])).reshape(-1) + 1
    if keep == "largest":
        keep = 1
    if isinstance(keep, bool) or not isinstance(keep, int) or keep < 0:
        raise ValueError(f"keep_components: keep must be 'largest', an int or ('min_voxels', m), got {keep!r}")
    order = torch.sort(sizes, descending=True, stable=True).indices       # (stable: equal sizes stay in label order)
    return torch.sort(order[:min(keep, n)]).values + 1


def keep_components(volume, isovalue, keep, return_sizes=False):
    """Drops solid components from a device fp64 volume: (filtered fp64 volume, kept labels int64).  Every voxel of a dropped component
    gets iso + |v - iso| (the next double above iso where that is not above iso); every other voxel is copied bit for bit.  The
    corners of a marching-cubes cell are pairwise 26-adjacent, so a rewritten value never meets a kept solid corner in a cell: the
    mesh of the kept components does not change.  return_sizes: also the sizes of all components before filtering."""
    v = _volume(volume, (torch.float64,), "keep_components")
    labels, sizes = label_components(v, isovalue)
    kept = select_components(sizes, keep)
    out = filter_components(v, isovalue, labels, int(sizes.numel()), kept)
    return (out, kept, sizes) if return_sizes else (out, kept)


def filter_components(volume, isovalue, labels, n_labels, kept):
    """The filter step of keep_components alone: `labels` as label_components returned them for this volume and isovalue, `kept` the
    labels (int64, 1-based) that stay."""
    v = _volume(volume, (torch.float64,), "filter_components")
    if labels.dtype != torch.int32 or labels.shape != v.shape or labels.device != v.device:
        raise ValueError("filter_components: labels must be the int32 device volume label_components returned")
    mask = torch.zeros(max(n_labels, 1), dtype=torch.uint8, device=v.device)
    mask[kept - 1] = 1
    out = torch.empty_like(v)
    with _lib.on(v.device):
        _lib.check(_lib.lib().hl_cc_filter(_dptr(v), _dptr(labels.contiguous()), _dptr(mask), v.numel(), n_labels, float(isovalue), _dptr(out),
                                           _lib.stream_ptr(v.device)), "hl_cc_filter")
    return out


def case_table():
    """The baked marching-cubes table: list over the 256 corner configurations of [(e0, e1, e2), ...] cube edges."""
    import ctypes as C
    L = _lib.lib()
    mt = L.hl_mc_max_triangles()
    tris = np.zeros((256, mt, 3), dtype=np.int8)
    ntri = np.zeros(256, dtype=np.uint8)
    _lib.check(L.hl_mc_case_table(tris.ctypes.data_as(C.c_void_p), ntri.ctypes.data_as(C.c_void_p)), "hl_mc_case_table")
    return [[tuple(int(e) for e in tris[c, t]) for t in range(ntri[c])] for c in range(256)]


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """Binary little-endian PLY: float64 vertices, one (uchar 3, int32 x3) list per face.  With `normals` (V,3) and / or `colors`
    (V,3) uint8 the vertex element also carries `float nx ny nz` and / or `uchar red green blue`; without them the file is what it
    always was.  The reference writes its meshes with trimesh, which this package does not depend on; any PLY reader loads this."""
    v = np.ascontiguousarray(np.asarray(_host(vertices), dtype="<f8").reshape(-1, 3))
    t = _host(triangles).reshape(-1, 3)
    if len(v) and t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("write_ply: triangle index out of range")
    fields, props = [("p", "<f8", (3,))], "property double x\nproperty double y\nproperty double z\n"
    if normals is not None:
        fields.append(("n", "<f4", (3,)))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        fields.append(("c", "u1", (3,)))
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    vert = np.empty(len(v), dtype=fields)
    vert["p"] = v
    for key, arr, what in (("n", normals, "normals"), ("c", colors, "colors")):
        if arr is None:
            continue
        arr = _host(arr)
        if arr.shape != (len(v), 3):
            raise ValueError(f"write_ply: {what} must be (V,3) like the vertices, got {arr.shape}")
        if key == "c" and arr.dtype != np.uint8:
            raise TypeError(f"write_ply: colors must be uint8, got {arr.dtype}")
        vert[key] = arr
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {len(v)}\n{props}"
            f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    face = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    face["n"] = 3
    face["i"] = t
    with open(path, "wb") as f:
        f.write(head)
        f.write(vert.tobytes())
        f.write(face.tobytes())


def read_ply(path):
    """Reads back what write_ply wrote: (vertices float64 (V,3), triangles int64 (T,3)), followed by normals float32 (V,3) and / or
    colors uint8 (V,3) when the file has them."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nt = int(next(h for h in head if h.startswith("element face")).split()[-1])
    fields = [("p", "<f8", (3,))]
    if "property float nx" in head:
        fields.append(("n", "<f4", (3,)))
    if "property uchar red" in head:
        fields.append(("c", "u1", (3,)))
    vdt = np.dtype(fields)
    vert = np.frombuffer(data, dtype=vdt, count=nv, offset=end)
    face = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nt, offset=end + nv * vdt.itemsize)
    assert (face["n"] == 3).all()
    return (vert["p"].copy(), face["i"].astype(np.int64)) + tuple(vert[k].copy() for k in ("n", "c") if k in vdt.names)


def _dptr(t):
    """Device pointer of an fp64 / fp32 / byte tensor (the ABI's double* and void* arguments)."""
    return _lib.ptr(t, dtype=t.dtype)
