"""Animating an extracted mesh: bind its vertices to a posed body once, repose them for any frames (csrc/hl_mesh_animate.hip).

`Renderer.extract_mesh` gives the surface in the one pose it was extracted in.  Bound to the body of that pose, the mesh follows the
body through a sequence without another extraction - a gather and a 3x3 per vertex and frame instead of a density grid, a smoothing and
a marching-cubes pass.  Contract and formulas: DESIGN.md "Animating the mesh".

    posed = model.pose(poses, shapes, R, Th, forward_rows=True)       # the extraction pose and the sequence, rows kept
    mesh = renderer.extract_mesh(posed.tp_input(0), planes)
    binding = renderer.bind_mesh(mesh, posed, frame=0)                # or bind_mesh(mesh["vertices"], posed, normals=mesh["normals"])
    out = binding.repose(posed, frames=slice(0, 64))                  # vertices (F,N,3), normals (F,N,3), world_bounds (F,2,3)

Each mesh vertex is tied to its `neighbours` nearest body vertices with inverse-square-distance weights and stored in the blended rest
frame of those vertices; `neighbours=1` is the rule by which the canonical-space renderer deforms space (a rigid follow of the nearest
vertex), which tears the surface wherever the nearest vertex changes - hence the default of 4.  The body's shape offset stays inside the
stored rest position: reposing with other betas moves the joints with the new shape but keeps the bind frame's surface offset.

There is no CPU path: binding and reposing need device tensors and the HIP library.
"""
import torch

from .. import _lib
from . import mesh

MAX_NEIGHBOURS = 8


def _rows_of(posed, what):
    if getattr(posed, "rows", None) is None:
        raise ValueError(f"{what}: the posed body carries no forward rows; pose it with forward_rows=True")
    return posed.rows


def _points(what, a, dev):
    """(N,3) numpy array or device tensor of any dtype -> contiguous fp32 on `dev`."""
    mesh.refuse_cpu_tensor("bind_mesh", what, a)
    t = mesh.to_device(a, torch.float32, dev)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"bind_mesh: `{what}` must be (N,3), got {tuple(t.shape)}")
    return t


def bind_mesh(vertices, posed, frame=0, neighbours=4, normals=None):
    """vertices (N,3) world, normals (N,3) world or None: numpy arrays or device tensors of any float dtype (extract_mesh hands back
    fp64 numpy).  `posed`: a PosedBody made with forward_rows=True; `frame`: which of its frames the mesh was extracted in.
    -> MeshBinding."""
    rows = _rows_of(posed, "bind_mesh")
    model = posed.model
    K, V, F = int(neighbours), int(model.V), int(posed.F)
    if not 1 <= K <= MAX_NEIGHBOURS or K > V:
        raise ValueError(f"bind_mesh: neighbours must be 1 .. {min(MAX_NEIGHBOURS, V)} (a body of {V} vertices), got {neighbours}")
    frame = int(frame)
    if not 0 <= frame < F:
        raise ValueError(f"bind_mesh: frame {frame} of a posed body of {F} frames")
    if not rows.is_cuda:
        raise RuntimeError("bind_mesh needs the posed body on a CUDA(HIP) device; there is no CPU path")
    dev = rows.device
    pts = _points("vertices", vertices, dev)
    nrm = None if normals is None else _points("normals", normals, dev)
    N = int(pts.shape[0])
    if nrm is not None and int(nrm.shape[0]) != N:
        raise ValueError(f"bind_mesh: {N} vertices, {int(nrm.shape[0])} normals")
    b = MeshBinding()
    b.model, b.N, b.K, b.frame = model, N, K, frame
    b.ids = torch.empty((N, K), dtype=torch.int32, device=dev)
    b.weights = torch.empty((N, K), dtype=torch.float32, device=dev)
    b.rest = torch.empty((N, 3), dtype=torch.float32, device=dev)
    b.rest_normals = torch.empty((N, 3), dtype=torch.float32, device=dev) if nrm is not None else None
    rt = posed.rt[frame if posed.rt.shape[0] > 1 else 0]
    transl = getattr(posed, "transl", None)             # (SMPL-X adds it after skinning: verts4 holds it, the rows do not)
    transl = None if transl is None else transl[frame]
    with _lib.on(dev):
        _lib.check(_lib.lib().hl_mesh_bind(_lib.ptr(pts), _lib.ptr(nrm), N, _lib.ptr(posed.verts4[frame]), _lib.ptr(rows[frame]), V,
                                           _lib.ptr(rt), _lib.ptr(transl), K, _lib.ptr(b.ids, torch.int32), _lib.ptr(b.weights), _lib.ptr(b.rest),
                                           _lib.ptr(b.rest_normals), _lib.stream_ptr(dev)), "hl_mesh_bind")
    return b


class MeshBinding:
    """A mesh tied to a body model.  Device tensors: ids int32 (N,K) - the K nearest body vertices of every mesh vertex in the bind frame,
    by (distance, index) - weights (N,K) summing to 1, rest (N,3) - the vertex in the blended rest frame of its neighbours - and
    rest_normals (N,3) or None.  `model`: the body model it was bound to; N, K; `frame`: the bind frame.  `triangles`, `colors`: what
    Renderer.bind_mesh keeps alongside (they belong to the surface, not to the pose), else None."""
    triangles = colors = None

    def repose(self, posed, frames=None, normals=True, bounds=True, margin=0.05, y_margin=0.05):
        """The mesh in frames `frames` of `posed` (None: all; an int; a slice - so that a caller can bound the F N output): a dict of
        device tensors `vertices` (F,N,3) world, `normals` (F,N,3) unit, zero where the bound normal was zero (None without bound normals
        or with normals=False) and `world_bounds` (F,2,3): min / max of the frame's vertices, - / + margin, y once more by y_margin
        (None with bounds=False)."""
        rows = _rows_of(posed, "MeshBinding.repose")
        if posed.model is not self.model:
            raise ValueError("MeshBinding.repose: the posed body belongs to another body model than the one the mesh was bound to")
        if margin < 0 or y_margin < 0:
            raise ValueError(f"MeshBinding.repose: the bounds' margins must not be negative (got {margin}, {y_margin})")
        Fall = int(posed.F)
        if frames is None:
            frames = slice(0, Fall)
        elif isinstance(frames, slice):
            if frames.step not in (None, 1):
                raise ValueError("MeshBinding.repose: `frames` must be a slice of step 1 (the frames are read in place)")
            frames = slice(*frames.indices(Fall)[:2])
        else:
            f = int(frames)
            if not -Fall <= f < Fall:
                raise ValueError(f"MeshBinding.repose: frame {f} of a posed body of {Fall} frames")
            frames = slice(f % Fall, f % Fall + 1)
        F = frames.stop - frames.start
        if F < 1:
            raise ValueError(f"MeshBinding.repose: `frames` selects no frame of {Fall}")
        if not rows.is_cuda:
            raise RuntimeError("MeshBinding.repose needs the posed body on a CUDA(HIP) device; there is no CPU path")
        dev, N, K, V = rows.device, self.N, self.K, int(self.model.V)
        if self.ids.device != dev:
            raise ValueError(f"MeshBinding.repose: the binding is on {self.ids.device}, the posed body on {dev}")
        want_normals = bool(normals) and self.rest_normals is not None
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        out = {"vertices": new(F, N, 3), "normals": new(F, N, 3) if want_normals else None, "world_bounds": new(F, 2, 3) if bounds else None}
        if N == 0:
            if bounds:      # (the min / max of no vertices, as the kernel would leave them)
                out["world_bounds"][:, 0], out["world_bounds"][:, 1] = float("inf"), float("-inf")
            return out
        per_frame = posed.rt.shape[0] > 1
        rt = posed.rt[frames] if per_frame else posed.rt
        transl = getattr(posed, "transl", None)
        transl = None if transl is None else transl[frames]
        L = _lib.lib()
        with _lib.on(dev):
            scratch = new(L.hl_mesh_repose_scratch_bytes(N, F) // 4) if bounds else None
            _lib.check(L.hl_mesh_repose(_lib.ptr(self.ids, torch.int32), _lib.ptr(self.weights), _lib.ptr(self.rest),
                                        _lib.ptr(self.rest_normals) if want_normals else None, N, K, _lib.ptr(rows[frames]), V, F, _lib.ptr(rt),
                                        12 if per_frame else 0, _lib.ptr(transl), _lib.ptr(out["vertices"]), _lib.ptr(out["normals"]),
                                        _lib.ptr(out["world_bounds"]), float(margin), float(y_margin), _lib.ptr(scratch),
                                        scratch.numel() * 4 if bounds else 0, _lib.stream_ptr(dev)), "hl_mesh_repose")
        return out

    def rasterize(self, posed, H, W, K, R, T, frames=None, **kw):
        """repose(posed, frames), then raster.rasterize with the binding's triangles and colours: the mesh in those frames as images
        (rgb_map, acc_map, normal_map, depth_map, triangle_id, barycentrics, each (F,H,W,...)).  K, R, T: one camera for all frames or
        one per frame; `kw`: rasterize's options (shade, white_bkgd, cull, znear, check_indices).  DESIGN.md "Rasterising the mesh"."""
        from . import raster
        if self.triangles is None or len(self.triangles) == 0:
            raise ValueError("MeshBinding.rasterize: the binding carries no triangles (bind with Renderer.bind_mesh, or set `triangles`)")
        moved = self.repose(posed, frames=frames, bounds=False)
        dev = moved["vertices"].device
        cached = getattr(self, "_triangles_i32", None)      # (triangles, its int32 device copy): converted once, not per call
        if cached is None or cached[0] is not self.triangles or cached[1].device != dev:
            cached = self._triangles_i32 = (self.triangles, mesh.device_triangles(self.triangles, dev))
        return raster.rasterize(moved["vertices"], cached[1], H, W, K, R, T, normals=moved["normals"], colors=self.colors, **kw)
