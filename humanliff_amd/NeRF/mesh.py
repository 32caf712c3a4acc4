"""The input layer of the mesh stages (simplify, distance, raster, animate): what a mesh argument may be, how it reaches the device and
how the small read-backs come home.  Plain functions; the first argument `who` is the caller's name for the messages.  DESIGN.md "What
the mesh stages share"."""
import numpy as np
import torch

from .. import _lib


def is_float(a):
    return a.dtype.is_floating_point if torch.is_tensor(a) else np.issubdtype(a.dtype, np.floating)


def is_int(a):
    if torch.is_tensor(a):
        return not (a.dtype.is_floating_point or a.dtype.is_complex or a.dtype == torch.bool)
    return np.issubdtype(a.dtype, np.integer)


def refuse_cpu_tensor(who, what, a):
    if torch.is_tensor(a) and not a.is_cuda:
        raise RuntimeError(f"{who}: `{what}` is a CPU tensor; there is no CPU path (pass a numpy array or a device tensor)")


def _array(a):
    return a if a is None or torch.is_tensor(a) else np.asarray(a)


def mesh_arrays(who, mesh_or_vertices, triangles, normals=None, colors=None, *, dict_extras=False, frames=False, any_dtype=False):
    """A mesh dict or vertices with `triangles` beside them -> (vertices, triangles, normals | None, colors | None, N, T): numpy arrays
    or device tensors, checked without a device.  vertices float (N,3), triangles integer (T,3), 1 <= N, T < 2^31, normals float
    (N,3), colors uint8 (N,3).  dict_extras: a dict's own `normals` and `colors` are used where none are given.  frames: rasterize's
    form - arrays only, vertices (N,3) or (F,N,3), normals (N,3), (1,N,3) or (F,N,3).  any_dtype: vertices and normals of any dtype."""
    if isinstance(mesh_or_vertices, dict) and not frames:
        if triangles is not None:
            raise ValueError(f"{who}: pass a mesh dict or (vertices, triangles), not both")
        mesh = mesh_or_vertices
        if "vertices" not in mesh or "triangles" not in mesh:
            raise ValueError(f"{who}: a mesh dict needs `vertices` and `triangles`")
        vertices, triangles = mesh["vertices"], mesh["triangles"]
        if dict_extras:
            normals = mesh.get("normals") if normals is None else normals
            colors = mesh.get("colors") if colors is None else colors
    else:
        vertices = mesh_or_vertices
        if triangles is None:
            raise ValueError(f"{who}: `triangles` is missing")
    for what, a in (("vertices", vertices), ("triangles", triangles), ("normals", normals), ("colors", colors)):
        refuse_cpu_tensor(who, what, a)
    vertices, triangles = (a if torch.is_tensor(a) else np.asarray(a) for a in (vertices, triangles))
    normals, colors = _array(normals), _array(colors)
    lead = "(N,3) or (F,N,3)" if frames else "(N,3)"
    kind = "" if any_dtype else "float "
    vshape, tshape = tuple(vertices.shape), tuple(triangles.shape)
    if len(vshape) not in ((2, 3) if frames else (2,)) or vshape[-1] != 3 or not (any_dtype or is_float(vertices)):
        raise ValueError(f"{who}: `vertices` must be {kind}{lead}, got {vertices.dtype} {vshape}")
    if len(tshape) != 2 or tshape[1] != 3 or not is_int(triangles):
        raise ValueError(f"{who}: `triangles` must be (T,3) of an integer dtype, got {triangles.dtype} {tshape}")
    F, N, T = (1 if len(vshape) == 2 else vshape[0]), vshape[-2], tshape[0]
    if not (1 <= N < 1 << 31 and 1 <= T < 1 << 31 and F >= 1):
        raise ValueError(f"{who}: {N} vertices and {T} triangles (each 1 .. 2^31 - 1){'' if F else ' in no frame'}")
    if normals is not None:
        nshape = tuple(normals.shape)
        if not (nshape == (N, 3) or (frames and nshape in ((1, N, 3), (F, N, 3)))) or not (any_dtype or is_float(normals)):
            raise ValueError(f"{who}: `normals` must be {kind}({N},3){f', (1,{N},3) or ({F},{N},3)' if frames else ''}, got {normals.dtype} {nshape}")
    if colors is not None and (tuple(colors.shape) != (N, 3) or colors.dtype not in (torch.uint8, np.uint8)):
        raise ValueError(f"{who}: `colors` must be uint8 ({N},3), got {colors.dtype} {tuple(colors.shape)}")
    return vertices, triangles, normals, colors, N, T


def float_rows(who, what, a, rows=None):
    """Query points or normals: float (Q,3), exactly `rows` of them where given, numpy or device tensor."""
    refuse_cpu_tensor(who, what, a)
    a = _array(a)
    shape = tuple(a.shape)
    if len(shape) != 2 or shape[1] != 3 or not is_float(a) or (rows is not None and shape[0] != rows):
        raise ValueError(f"{who}: `{what}` must be float ({'Q' if rows is None else rows},3), got {a.dtype} {shape}")
    if shape[0] >= 1 << 31:
        raise ValueError(f"{who}: {shape[0]} rows in `{what}` (at most 2^31 - 1)")
    return a


def need_device(who):
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} needs a CUDA(HIP) device; there is no CPU path")


def device_of(*arrays):
    """The device of the first tensor among the arguments, else the current one."""
    return next((a.device for a in arrays if torch.is_tensor(a)), None) or torch.device("cuda", torch.cuda.current_device())


def to_device(a, dtype, dev):
    """numpy array or tensor -> contiguous `dtype` on `dev`."""
    t = a.detach() if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype).contiguous()


def device_triangles(triangles, dev):
    """(T,3) of any integer dtype, numpy array or device tensor -> contiguous int32 on `dev`.  An index that does not fit int32 is out of
    range whatever N is: it becomes -1, which the stages skip and flag.  An int32 device tensor passes through untouched, so a caller
    that rasterises the same triangles again and again converts them once with this and hands the result in."""
    tri = (triangles.detach() if torch.is_tensor(triangles) else torch.as_tensor(np.ascontiguousarray(triangles).astype(np.int64))).to(device=dev)
    if tri.dtype != torch.int32:
        tri = tri.to(torch.int64)
        tri = torch.where((tri < 0) | (tri >= 1 << 31), torch.full_like(tri, -1), tri).to(torch.int32)
    return tri.contiguous()


def dptr(t):
    """A device tensor or None -> its pointer, typed by its own dtype."""
    return _lib.ptr(t, None if t is None else t.dtype)


def finite_bounds(verts, origin=None):
    """Device vertices fp64 (N,3) -> (lo, hi) float64 (3,) over the vertices that are finite and, with an `origin` (float64 (3,)), at or
    above it; None when there is no such vertex.  One launch of the simplifier's bounds pass and one read-back."""
    dev = verts.device
    bounds = torch.empty(_lib.HL_SIMPLIFY_BOUNDS_WORDS, dtype=torch.float64, device=dev)
    with _lib.on(dev):
        _lib.check(_lib.lib().hl_mesh_simplify_bounds(dptr(verts), int(verts.shape[0]), None if origin is None else origin.ctypes.data, dptr(bounds),
                                                      _lib.stream_ptr(dev)), "hl_mesh_simplify_bounds")
    b = bounds[:6].cpu().numpy()
    return (np.ascontiguousarray(b[:3]), np.ascontiguousarray(b[3:])) if np.isfinite(b).all() else None


def grid_extents(lo, hi, cell, origin, max_cells, who):
    """Valid vertices between `lo` and `hi` (float64 (3,)) -> (origin, extents g int64 (3,)): origin = lo when none is given,
    g = floor((hi - origin) / cell) + 1 per axis - the arithmetic of the kernels, which is monotone in the coordinate, so no vertex
    lies past the extents.  ValueError for a grid of more than `max_cells` (a power of two) cells."""
    origin = lo.copy() if origin is None else origin
    cap = f"2^{max_cells.bit_length() - 1}"
    q = (hi - origin) / cell
    if not np.isfinite(q).all() or (q >= max_cells).any():
        raise ValueError(f"{who}: the grid of cell {np.asarray(cell).tolist()} over the vertices holds more than {cap} cells; use a larger cell")
    g = np.floor(q).astype(np.int64) + 1
    if int(g[0]) * int(g[1]) * int(g[2]) > max_cells:
        raise ValueError(f"{who}: a grid of {g.tolist()} cells holds more than {cap}; use a larger cell")
    return origin, g


def read_counts(words, k, joined=()):
    """Device int64 words - `k` counts and, where there are more, a word whose first int32 is the status -> (the counts as Python
    ints, the status or None), in one read-back.  joined: the places i where words i and i + 1 are the low and high 32 bits of one
    count, which is returned at i."""
    w = words.cpu()
    counts = w[:k].tolist()
    for i in joined:
        counts[i] |= counts[i + 1] << 32
    return counts, int(w[k:].view(torch.int32)[0]) if w.numel() > k else None
