"""Measuring the distance between meshes on the device: the exact closest triangle (csrc/hl_mesh_distance.hip).

For every query point the closest point of a triangle mesh - not of its vertices: a simplified mesh has triangles many vertex spacings
wide - found through a uniform grid of cubic cells, exactly; a deterministic area-weighted surface sampler; and on top of the two the
usual scores between two surfaces.  Contract and rules: DESIGN.md "Measuring mesh distance".

    hit = distance.point_mesh_distance(points, mesh)                # mesh: the dict extract_mesh / simplify_mesh returns
    hit["distance"] (Q,) fp64, hit["triangle"] (Q,) int64, hit["barycentric"] (Q,3), hit["point"] (Q,3), ...
    index = distance.build_index(mesh); index.query(points)         # the same, keeping the grid between calls
    pts = distance.sample_surface(mesh, 100_000)                    # points, triangle, barycentric, normals
    score = distance.mesh_distance(full, small, samples=100_000, thresholds=(0.005, 0.01))
    score["chamfer"], score["hausdorff"], score["fscore"], score["a_to_b"]["normal_consistency"], ...

All geometry is float64 relative to the lower corner of the target's bounds, in a fixed order of operations; between triangles the
smallest (squared distance, index) wins.  So a result does not depend on the cell size, on the order in which triangles are visited or
on scheduling, and has the same bits on every run.  There is no CPU path, no sign (inside / outside) and no gradient.
"""
import math

import numpy as np
import torch

from .. import _lib
from . import mesh

MAX_CELLS = 1 << 27
DEFAULT_CELLS = 1 << 24
MAX_REFS = 1 << 31
MAX_THRESHOLDS = 8
STATUS_INDEX, STATUS_CORNER, STATUS_QUERY = 1, 2, 4
_dp = mesh.dptr
REDUCE_FIELDS = ("sum_distance", "sum_sqdist", "sum_normal_dot", "count_normal_dot", "max", "count")


def _positive(who, what, x, allow_inf=False):
    if x is None:
        return None
    try:
        x = float(x)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{who}: `{what}` must be a number, got {x!r}") from e
    if not (x > 0.0 and (allow_inf or math.isfinite(x))):
        raise ValueError(f"{who}: `{what}` must be positive{'' if allow_inf else ' and finite'}, got {x}")
    return x


def _thresholds(who, thresholds):
    th = [float(t) for t in thresholds]
    if len(th) > MAX_THRESHOLDS:
        raise ValueError(f"{who}: {len(th)} thresholds, at most {MAX_THRESHOLDS}")
    if not all(math.isfinite(t) and t >= 0.0 for t in th):
        raise ValueError(f"{who}: `thresholds` must be finite and >= 0, got {th}")
    return th


def _validate(points, mesh_or_vertices, triangles=None, normals=None, cell=None, max_distance=None, thresholds=()):
    """Everything point_mesh_distance and mesh_distance can refuse without a device -> (points or None, vertices, triangles,
    normals or None, cell or None, max_distance or None, thresholds)."""
    who = "point_mesh_distance"
    vertices, triangles = mesh.mesh_arrays(who, mesh_or_vertices, triangles)[:2]
    if points is not None:
        points = mesh.float_rows(who, "points", points)
    if normals is not None:
        if points is None:
            raise ValueError(f"{who}: `normals` without `points`")
        normals = mesh.float_rows(who, "normals", normals, rows=int(points.shape[0]))
    return (points, vertices, triangles, normals, _positive(who, "cell", cell), _positive(who, "max_distance", max_distance, allow_inf=True),
            _thresholds("mesh_distance", thresholds))


def default_cell(area, T, longest, lo, hi):
    """h = max(2 sqrt(A / T), longest / 1024), raised by quarters until the grid over lo .. hi holds at most 2^24 cells."""
    h = max(2.0 * math.sqrt(area / T), longest / 1024.0)
    if not (h > 0.0 and math.isfinite(h)):
        h = 1.0                                     # a mesh without extent: one cell
    while True:
        g = np.floor((hi - lo) / h).astype(np.int64) + 1
        if int(g[0]) * int(g[1]) * int(g[2]) <= DEFAULT_CELLS:
            return h
        h *= 1.25


class MeshIndex:
    """The grid over a target mesh: the triangle records, the cell lists and the wide list, on the device.  `info`: N, T, valid, wide,
    references, extents, status.  Build it with build_index."""

    def __init__(self, verts, tri, origin, lo, hi, cell, check):
        dev = verts.device
        self.device, self.vertices, self.triangles = dev, verts, tri
        self.origin, self.lo, self.hi, self.cell = origin, lo, hi, float(cell)
        N, T = int(verts.shape[0]), int(tri.shape[0])
        gx, gy, gz = (int(x) for x in mesh.grid_extents(lo, hi, self.cell, origin, MAX_CELLS, "build_index")[1])
        self.extents = (gx, gy, gz)
        L = _lib.lib()
        need = int(L.hl_mesh_distance_scratch_bytes(T, gx, gy, gz))
        if need == 0:
            raise ValueError(f"build_index: sizes the library refuses (T {T}, grid {gx} x {gy} x {gz})")
        self.scratch = torch.empty(need // 4, dtype=torch.int32, device=dev)
        self.scratch_bytes = need
        words = torch.empty(6, dtype=torch.int64, device=dev)          # counts (4), then the status word
        counts, status = words[:4], words[4:].view(torch.int32)
        with _lib.on(dev):
            st = _lib.stream_ptr(dev)
            _lib.check(L.hl_mesh_distance_count(_dp(verts), N, _dp(tri), T, origin.ctypes.data, self.cell, gx, gy, gz, _dp(counts), _dp(status),
                                                _dp(self.scratch), need, st), "hl_mesh_distance_count")
            (refs, _, wide, valid), flags = mesh.read_counts(words, 4, joined=(0,))
            self.info = {"N": N, "T": T, "valid": valid, "wide": wide, "references": refs, "extents": self.extents, "status": flags}
            if check and flags & STATUS_INDEX:
                raise ValueError(f"build_index: `triangles` holds an index outside [0, {N}) (check=False drops such triangles)")
            if check and flags & STATUS_CORNER:
                raise ValueError("build_index: a triangle has a non-finite corner (check=False drops such triangles)")
            if valid == 0:
                raise ValueError("build_index: the target has no valid triangle")
            if wide > _lib.HL_DISTANCE_MAX_WIDE:
                raise ValueError(f"build_index: {wide} triangles cover more than {_lib.HL_DISTANCE_WIDE_CELLS} cells each, at most "
                                 f"{_lib.HL_DISTANCE_MAX_WIDE}; pass a larger `cell`")
            if refs > MAX_REFS:
                raise ValueError(f"build_index: {refs} cell references, at most 2^31; pass a larger `cell`")
            self.refs = torch.empty(max(refs, 1), dtype=torch.int32, device=dev)
            _lib.check(L.hl_mesh_distance_fill(T, origin.ctypes.data, self.cell, gx, gy, gz, _dp(self.refs), refs, _dp(self.scratch), need, st),
                       "hl_mesh_distance_fill")

    def query(self, points, normals=None, max_distance=None, check=True):
        """points (Q,3), normals (Q,3) or None: numpy arrays or device tensors of any float dtype -> the dict point_mesh_distance
        returns."""
        who = "MeshIndex.query"
        points = mesh.float_rows(who, "points", points)
        Q = int(points.shape[0])
        if normals is not None:
            normals = mesh.float_rows(who, "normals", normals, rows=Q)
        max_distance = _positive(who, "max_distance", max_distance, allow_inf=True)
        dev = self.device
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
        out = {"distance": f64(Q), "sqdist": f64(Q), "triangle": None, "barycentric": f64(Q, 3), "point": f64(Q, 3),
               "normal_dot": None if normals is None else f64(Q), "cell": self.cell, "origin": self.origin,
               "status": torch.full((1,), self.info["status"], dtype=torch.int32, device=dev),          # the target's bits; the query ors its own in
               "info": self.info}
        if Q == 0:
            out["triangle"] = torch.empty(0, dtype=torch.int64, device=dev)
            return out
        pts = mesh.to_device(points, torch.float64, dev)
        nrm = None if normals is None else mesh.to_device(normals, torch.float64, dev)
        tri = torch.empty(Q, dtype=torch.int32, device=dev)
        status = out["status"]
        gx, gy, gz = self.extents
        with _lib.on(dev):
            _lib.check(_lib.lib().hl_mesh_distance_query(
                _dp(pts), _dp(nrm), Q, self.info["T"], self.origin.ctypes.data, self.cell, gx, gy, gz, _dp(self.refs), self.info["references"],
                self.info["wide"], math.inf if max_distance is None else max_distance, _dp(out["sqdist"]), _dp(out["distance"]), _dp(tri),
                _dp(out["barycentric"]), _dp(out["point"]), _dp(out["normal_dot"]), _dp(status), _dp(self.scratch), self.scratch_bytes,
                _lib.stream_ptr(dev)), "hl_mesh_distance_query")
        out["triangle"], out["status"] = tri.to(torch.int64), status
        if check and int(status.item()) & STATUS_QUERY:
            raise ValueError("point_mesh_distance: `points` holds a non-finite coordinate (check=False gives such a query NaN and -1)")
        return out


def _bounds(verts):
    """Device vertices -> (lo, hi) float64 (3,) of the finite ones."""
    b = mesh.finite_bounds(verts)
    if b is None:
        raise ValueError("mesh distance: no vertex of the mesh is finite")
    return b


class _Areas:
    """The fixed-point areas of a mesh on the device: the exclusive prefix, the total A_fix, the unit u and A = A_fix u."""

    def __init__(self, verts, tri, lo, hi):
        dev = verts.device
        N, T = int(verts.shape[0]), int(tri.shape[0])
        self.longest = float((hi - lo).max())
        self.unit = (self.longest * self.longest) / 1073741824.0
        self.prefix = torch.zeros(T, dtype=torch.int64, device=dev)
        self.total = 0
        if not (self.unit > 0.0 and math.isfinite(self.unit)):
            self.area = 0.0
            return                                  # a mesh without extent has no area
        nb = (T + 4095) // 4096
        blocks = torch.empty(nb, dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        with _lib.on(dev):
            _lib.check(_lib.lib().hl_mesh_distance_areas(_dp(verts), N, _dp(tri), T, lo.ctypes.data, self.unit, _dp(self.prefix), _dp(counts), _dp(blocks),
                                                         nb * 8, _lib.stream_ptr(dev)), "hl_mesh_distance_areas")
        self.total = mesh.read_counts(counts, 2, joined=(0,))[0][0]
        self.area = self.total * self.unit


def _device_mesh(who, mesh_or_vertices, triangles):
    """-> (vertices fp64, triangles int32 on the device, the dict's `normals` as given or None)."""
    vertices, triangles = mesh.mesh_arrays(who, mesh_or_vertices, triangles)[:2]
    mesh.need_device(who)
    dev = mesh.device_of(vertices, triangles)
    normals = mesh_or_vertices.get("normals") if isinstance(mesh_or_vertices, dict) else None
    return mesh.to_device(vertices, torch.float64, dev), mesh.device_triangles(triangles, dev), normals


def build_index(mesh_or_vertices, triangles=None, *, cell=None, check=True):
    """The grid over a target mesh, to be queried again and again -> MeshIndex.  cell: the side of the cubic cells in world units, or
    None: max(2 sqrt(area / T), longest side of the bounds / 1024), raised until the grid holds at most 2^24 cells.  The answers do
    not depend on it; the time does."""
    cell = _positive("build_index", "cell", cell)
    verts, tri, _ = _device_mesh("build_index", mesh_or_vertices, triangles)
    lo, hi = _bounds(verts)
    if cell is None:
        ar = _Areas(verts, tri, lo, hi)
        cell = default_cell(ar.area, int(tri.shape[0]), ar.longest, lo, hi)
    return MeshIndex(verts, tri, lo.copy(), lo, hi, cell, check)


def point_mesh_distance(points, mesh_or_vertices, triangles=None, *, normals=None, cell=None, max_distance=None, check=True):
    """points (Q,3) and optionally their normals (Q,3) against the mesh (a dict with `vertices` and `triangles`, or the two arrays):
    numpy arrays or device tensors of any float dtype.  A target triangle with an index outside [0, N) or a non-finite corner is
    dropped and a query with a non-finite coordinate gets NaN and -1: with check=True (one status word read back) either raises
    ValueError instead.  max_distance: a query farther than this gets distance inf and triangle -1, and the search stops early.
    -> dict of device tensors: `distance` fp64 (Q,) = sqrt(`sqdist`), `triangle` int64 (Q,), `barycentric` and `point` fp64 (Q,3),
    `normal_dot` fp64 (Q,) or None: the cosine between the query's normal and the hit triangle's (NaN for a degenerate hit or a zero
    normal); `cell` and `origin` as used; `status`: a device int32 (1,) with the bits STATUS_INDEX, STATUS_CORNER, STATUS_QUERY; `info`:
    the index's counts (valid and wide triangles, references, extents)."""
    points, vertices, triangles, normals, cell, max_distance, _ = _validate(points, mesh_or_vertices, triangles, normals, cell, max_distance)
    if points is None:
        raise ValueError("point_mesh_distance: `points` is missing")
    index = build_index(vertices, triangles, cell=cell, check=check)
    return index.query(points, normals, max_distance, check=check)


def sample_surface(mesh_or_vertices, samples, triangles=None, *, seed=0):
    """`samples` points on the mesh's triangles, area-weighted and deterministic: sample s lies in the triangle that holds position
    (s + 0.5) / samples of the running area, at barycentrics from the R2 low-discrepancy sequence; `seed` (0 .. 2^32 - 1) picks another
    stretch of the sequence.  -> dict of device tensors: `points` fp64 (S,3), `triangle` int64 (S,), `barycentric` fp64 (S,3), `normals`
    fp64 (S,3): the unit face normal.  A triangle without area is never chosen; a mesh without area raises ValueError."""
    who = "sample_surface"
    S, seed = int(samples), int(seed)
    if not 1 <= S < 1 << 31:
        raise ValueError(f"{who}: `samples` must be 1 .. 2^31 - 1, got {samples}")
    if not 0 <= seed < 1 << 32:
        raise ValueError(f"{who}: `seed` must be 0 .. 2^32 - 1, got {seed}")
    verts, tri, _ = _device_mesh(who, mesh_or_vertices, triangles)
    lo, hi = _bounds(verts)
    return _sample(verts, tri, lo, _Areas(verts, tri, lo, hi), S, seed)


def _sample(verts, tri, lo, ar, S, seed):
    if ar.total == 0:
        raise ValueError("sample_surface: the mesh has no area")
    dev = verts.device
    f64 = lambda: torch.empty((S, 3), dtype=torch.float64, device=dev)  # noqa: E731
    out = {"points": f64(), "triangle": torch.empty(S, dtype=torch.int64, device=dev), "barycentric": f64(), "normals": f64()}
    with _lib.on(dev):
        _lib.check(_lib.lib().hl_mesh_distance_sample(_dp(verts), int(verts.shape[0]), _dp(tri), int(tri.shape[0]), lo.ctypes.data, _dp(ar.prefix), ar.total,
                                                      S, seed, _dp(out["points"]), _dp(out["triangle"]), _dp(out["barycentric"]), _dp(out["normals"]),
                                                      _lib.stream_ptr(dev)), "hl_mesh_distance_sample")
    return out


def reduce_queries(hit, thresholds=()):
    """The fixed-order sums over one side's queries (a dict as point_mesh_distance returns it) -> dict: count, mean, mean_sq, rms,
    max, within (a fraction per threshold), normal_consistency or None.  One read-back."""
    th = _thresholds("mesh_distance", thresholds)
    d = hit["distance"]
    Q, dev = int(d.shape[0]), d.device
    if Q == 0:
        raise ValueError("mesh_distance: no queries")
    out = torch.empty(_lib.HL_DISTANCE_REDUCE_WORDS, dtype=torch.float64, device=dev)
    tha = np.ascontiguousarray(np.asarray(th + [0.0], dtype=np.float64))
    with _lib.on(dev):
        _lib.check(_lib.lib().hl_mesh_distance_reduce(_dp(d), _dp(hit["sqdist"]), _dp(hit["normal_dot"]), Q, tha.ctypes.data, len(th), _dp(out),
                                                      _lib.stream_ptr(dev)), "hl_mesh_distance_reduce")
    r = out[:_lib.HL_DISTANCE_REDUCE_FIELDS].cpu().tolist()
    n = int(r[5])
    if n == 0:
        raise ValueError("mesh_distance: no query has a finite distance")
    return {"count": n, "mean": r[0] / n, "mean_sq": r[1] / n, "rms": math.sqrt(r[1] / n), "max": r[4], "within": [r[8 + k] / n for k in range(len(th))],
            "normal_consistency": r[2] / r[3] if hit["normal_dot"] is not None and r[3] > 0 else None, "sums": dict(zip(REDUCE_FIELDS, r[:6]))}


def _side_queries(verts, tri, normals, samples, seed):
    """One mesh's queries: its vertices, then `samples` surface samples -> (points, normals or None).  Without vertex normals the
    vertices' rows of the normals are zero, which gives them no normal_dot."""
    if samples == 0:
        return verts, None if normals is None else mesh.to_device(normals, torch.float64, verts.device)
    lo, hi = _bounds(verts)
    smp = _sample(verts, tri, lo, _Areas(verts, tri, lo, hi), samples, seed)
    vn = torch.zeros_like(verts) if normals is None else mesh.to_device(normals, torch.float64, verts.device)
    return torch.cat([verts, smp["points"]]), torch.cat([vn, smp["normals"]])


def mesh_distance(a, b, *, samples=0, seed=0, thresholds=(), cell=None, check=True):
    """The distance scores between two meshes (dicts with `vertices`, `triangles` and optionally `normals`, or (vertices, triangles)
    pairs).  The queries of each side are its vertices plus, with samples > 0, that many surface samples; each is measured against
    the other mesh's surface.  -> dict of Python numbers: `a_to_b` and `b_to_a` (count, mean, mean_sq, rms, max, within: the fraction
    of queries within each threshold, normal_consistency: the mean cosine where it is defined, or None), `chamfer` = the two means
    added, `chamfer_sq` = the two mean squared distances added, `hausdorff` = the larger max, `fscore`: per threshold 2 P R / (P + R)
    with P = within of a_to_b and R = within of b_to_a."""
    th = _thresholds("mesh_distance", thresholds)
    cell = _positive("mesh_distance", "cell", cell)
    S, seed = int(samples), int(seed)
    if not 0 <= S < 1 << 31:
        raise ValueError(f"mesh_distance: `samples` must be 0 .. 2^31 - 1, got {samples}")
    if not 0 <= seed < 1 << 32:
        raise ValueError(f"mesh_distance: `seed` must be 0 .. 2^32 - 1, got {seed}")
    sides = []
    for m in (a, b):
        m = m if isinstance(m, dict) else {"vertices": m[0], "triangles": m[1]}
        verts, tri, normals = _device_mesh("mesh_distance", m, None)
        if normals is not None:
            normals = mesh.float_rows("mesh_distance", "normals", normals, rows=int(verts.shape[0]))
        sides.append((verts, tri, normals))
    out = {}
    for name, (src, dst) in (("a_to_b", (0, 1)), ("b_to_a", (1, 0))):
        pts, nrm = _side_queries(*sides[src], S, seed)
        index = build_index(sides[dst][0], sides[dst][1], cell=cell, check=check)
        out[name] = reduce_queries(index.query(pts, nrm, check=check), th)
    ab, ba = out["a_to_b"], out["b_to_a"]
    out["chamfer"] = ab["mean"] + ba["mean"]
    out["chamfer_sq"] = ab["mean_sq"] + ba["mean_sq"]
    out["hausdorff"] = max(ab["max"], ba["max"])
    out["thresholds"] = th
    out["fscore"] = [0.0 if p + r == 0.0 else 2.0 * p * r / (p + r) for p, r in zip(ab["within"], ba["within"])]
    return out
