"""Simplifying a mesh on the device: cell clustering with quadrics (csrc/hl_mesh_simplify.hip).

`Renderer.extract_mesh` gives the marching-cubes surface at the lattice's full density - about 500 000 vertices for a body at 512^3.
This turns it into a mesh whose vertex spacing the caller chooses: the vertices are clustered on a regular grid of cells, each
occupied cell gets one vertex, placed by the quadric error of the triangles that touch the cell (Lindstrom 2000), and the triangles
whose corners fall into three different cells remain, once per oriented triple.  Contract and rules: DESIGN.md "Simplifying the mesh".

    small = simplify.simplify_mesh(mesh, cell=0.02)                 # mesh: the dict extract_mesh returns
    small["vertices"] (V,3) fp64, small["triangles"] (T,3) int64, small["normals"], small["colors"], small["vertex_map"] (N,) int64

bind_mesh, rasterize and write_ply take the result as they take the full mesh.  Every accumulation is an integer sum, so the result
has the same bits on every run and does not depend on the order of the triangles (their output order apart) or of the vertices.

There is no CPU path, no target triangle count (the cell size is the control), no manifold repair (clustering can pinch a thin limb
into a non-manifold edge) and no gradient.
"""
import numpy as np
import torch

from .. import _lib
from . import mesh

MAX_CELLS = 1 << 31
MAX_CLUSTERS = 1 << 21
ACC_FIELDS = ("count", "px", "py", "pz", "nx", "ny", "nz", "r", "g", "b", "xx", "xy", "xz", "yy", "yz", "zz", "xd", "yd", "zd", "dd")
STATUS_VERTEX, STATUS_INDEX, STATUS_TABLE = 1, 2, 4


def _three(x, what):
    """A scalar or 3 numbers -> float64 (3,)."""
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    try:
        v = np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"simplify_mesh: `{what}` must be a number or 3 numbers, got {x!r}") from e
    if v.shape == ():
        v = np.full(3, float(v))
    if v.shape != (3,):
        raise ValueError(f"simplify_mesh: `{what}` must be a number or 3 numbers, got shape {v.shape}")
    return np.ascontiguousarray(v)


def _validate(mesh_or_vertices, triangles, cell, origin, normals, colors):
    """Everything that can be refused without a device -> (vertices, triangles, normals, colors, cell (3,), origin (3,) | None)."""
    vertices, triangles, normals, colors, _, _ = mesh.mesh_arrays("simplify_mesh", mesh_or_vertices, triangles, normals, colors, dict_extras=True)
    cell = _three(cell, "cell")
    if not (np.isfinite(cell).all() and (cell > 0).all()):
        raise ValueError(f"simplify_mesh: `cell` must be positive and finite, got {cell.tolist()}")
    if origin is not None:
        origin = _three(origin, "origin")
        if not np.isfinite(origin).all():
            raise ValueError(f"simplify_mesh: `origin` must be finite, got {origin.tolist()}")
    if not torch.is_tensor(vertices):
        # host vertices: the grid's size is known before anything reaches the device (the device pass below stays the authority)
        v = np.asarray(vertices, dtype=np.float64)
        ok = np.isfinite(v).all(axis=1)
        if origin is not None:
            ok &= (v >= origin[None]).all(axis=1)
        if ok.any():
            mesh.grid_extents(v[ok].min(axis=0), v[ok].max(axis=0), cell, origin, MAX_CELLS, "simplify_mesh")
    return vertices, triangles, normals, colors, cell, origin


def simplify_mesh(mesh_or_vertices, triangles=None, *, cell, origin=None, normals=None, colors=None, check=True):
    """mesh_or_vertices: the dict extract_mesh returns, or vertices (N,3) with `triangles` (T,3) of any integer dtype beside them;
    normals (N,3) and colors uint8 (N,3) are optional (a dict's own are used unless given): numpy arrays or device tensors, any float
    dtype.  cell: the cell size in world units, one number or one per axis.  origin: the grid's corner, 3 numbers, or None - the
    componentwise minimum of the vertices, found on the device.  A vertex with a non-finite coordinate or a coordinate below the
    origin belongs to no cell, and a triangle that uses one, or an index outside [0, N), is dropped: with check=True (one status word
    read back) either raises ValueError instead.
    -> dict of numpy arrays: `vertices` fp64 (V,3), `triangles` int64 (T',3), `normals` fp64 (V,3) or None, `colors` uint8 (V,3) or
    None, `vertex_map` int64 (N,): the output vertex of every input vertex or -1, `cell` and `origin` fp64 (3,) as used.  A mesh that
    lies inside one cell gives 0 vertices and 0 triangles."""
    out, _, _ = _simplify(mesh_or_vertices, triangles, cell=cell, origin=origin, normals=normals, colors=colors, check=check)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def _simplify(mesh_or_vertices, triangles=None, *, cell, origin=None, normals=None, colors=None, check=True, alloc=None):
    """simplify_mesh's body -> (outputs as device tensors, scratch as int32 words or None when nothing was launched into it, info:
    N, T, clusters, extents, status).  `alloc(shape, dtype)`, default torch.empty on the device, provides the five outputs at their
    upper bounds and then the scratch, in that order."""
    vertices, triangles, normals, colors, cell, origin = _validate(mesh_or_vertices, triangles, cell, origin, normals, colors)
    mesh.need_device("simplify_mesh")
    dev = mesh.device_of(vertices, triangles, normals, colors)
    N, T = int(vertices.shape[0]), int(triangles.shape[0])
    verts = mesh.to_device(vertices, torch.float64, dev)
    nrm = None if normals is None else mesh.to_device(normals, torch.float64, dev)
    col = None if colors is None else mesh.to_device(colors, torch.uint8, dev)
    tri = mesh.device_triangles(triangles, dev)
    if alloc is None:
        alloc = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    L = _lib.lib()
    dp = mesh.dptr
    info = {"N": N, "T": T, "clusters": 0, "extents": None, "status": 0}

    def result(v, t, n, c, vmap, org):
        return {"vertices": v, "triangles": t, "normals": n, "colors": c, "vertex_map": vmap, "cell": cell, "origin": org}

    def empty(org):
        z = lambda dt: torch.zeros((0, 3), dtype=dt, device=dev)  # noqa: E731
        return result(z(torch.float64), z(torch.int64), None if nrm is None else z(torch.float64), None if col is None else z(torch.uint8),
                      torch.full((N,), -1, dtype=torch.int64, device=dev), org)

    with _lib.on(dev):
        st = _lib.stream_ptr(dev)
        b = mesh.finite_bounds(verts, origin)
        if b is None:                                # no vertex has a cell
            if check:
                raise ValueError("simplify_mesh: no vertex is finite and at or above `origin`")
            info["status"] = STATUS_VERTEX
            return empty(np.zeros(3) if origin is None else origin), None, info
        origin, g = mesh.grid_extents(*b, cell, origin, MAX_CELLS, "simplify_mesh")
        gx, gy, gz = (int(x) for x in g)
        info["extents"] = (gx, gy, gz)
        need = int(L.hl_mesh_simplify_scratch_bytes(N, T, gx, gy, gz))
        if need == 0:
            raise ValueError(f"simplify_mesh: sizes the library refuses (N {N}, T {T}, grid {gx} x {gy} x {gz})")
        bound_v = min(N, gx * gy * gz, MAX_CLUSTERS)
        out_v = alloc((bound_v, 3), torch.float64)
        out_t = alloc((T, 3), torch.int64)
        out_n = None if nrm is None else alloc((bound_v, 3), torch.float64)
        out_c = None if col is None else alloc((bound_v, 3), torch.uint8)
        vmap = alloc((N,), torch.int64)
        scratch = alloc((need // 4,), torch.int32)
        assert scratch.numel() * 4 == need and scratch.is_contiguous()
        words = torch.empty(8, dtype=torch.int64, device=dev)          # counts (6), then the status word
        counts, status = words[:6], words[6:].view(torch.int32)
        _lib.check(L.hl_mesh_simplify_count(dp(verts), N, T, cell.ctypes.data, origin.ctypes.data, gx, gy, gz, dp(counts), dp(status), dp(scratch),
                                            need, st), "hl_mesh_simplify_count")
        clusters = int(counts[0].item())
        info["clusters"] = clusters
        if clusters > MAX_CLUSTERS:
            raise ValueError(f"simplify_mesh: {clusters} occupied cells, at most 2^21; use a larger cell")
        assert 1 <= clusters <= bound_v
        _lib.check(L.hl_mesh_simplify_emit(dp(verts), dp(nrm), dp(col), N, dp(tri), T, cell.ctypes.data, origin.ctypes.data, gx, gy, gz, clusters,
                                           dp(out_v), dp(out_n), dp(out_c), dp(out_t), dp(vmap), dp(counts), dp(status), dp(scratch), need, st),
                   "hl_mesh_simplify_emit")
        (_, _, n_tri, _, n_vert, _), flags = mesh.read_counts(words, 6)
    info["status"] = flags
    if flags & STATUS_TABLE:
        raise RuntimeError("simplify_mesh: the duplicate table ran out of probes")       # (half empty by construction: cannot happen)
    if check and flags & STATUS_VERTEX:
        raise ValueError("simplify_mesh: `vertices` holds a non-finite coordinate or one below `origin` (check=False drops its triangles)")
    if check and flags & STATUS_INDEX:
        raise ValueError(f"simplify_mesh: `triangles` holds an index outside [0, {N}) (check=False drops such triangles)")
    return result(out_v[:n_vert], out_t[:n_tri], None if out_n is None else out_n[:n_vert], None if out_c is None else out_c[:n_vert], vmap,
                  origin), scratch, info


def scratch_cluster_ids(scratch, N):
    """The cluster id of every input vertex inside a scratch of hl_mesh_simplify_emit, for inspection (its fixed layout begins with
    them): int32 (N,), -1 for a vertex without a cell.  Ids ascend with the cell key (cz gy + cy) gx + cx."""
    return scratch[:N]


def scratch_accumulators(scratch, N, clusters):
    """The integer accumulators inside a scratch of hl_mesh_simplify_emit, for inspection: int64 (clusters, 20) in the order of
    ACC_FIELDS, fixed point at 2^30 per unit except the count and the colour sums."""
    o = (N * 4 + 15) // 16 * 4
    return scratch[o:o + clusters * _lib.HL_SIMPLIFY_ACC_WORDS * 2].view(torch.int64).view(clusters, _lib.HL_SIMPLIFY_ACC_WORDS)
