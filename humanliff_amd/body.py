"""The body model on the device: loading an SMPL-style asset and posing it with the hl_body_* kernels (csrc/hl_body.hip).

The reference poses the body in its dataset code with numpy (smpl/smpl_numpy.py, SynBodyView_datasets.py:141-194) and rebuilds the
per-point deformation inputs with stock PyTorch ops.  Here one call poses a frame or a whole sequence: posed vertices, joints and
world bounds as `prepare_input` returns them, plus the (verts4, table) pair hl_deform_points / hl_deform_rays consume, so that a
renderer handed `tp_input['deform']` runs no torch op chain and reads nothing back per view.  Contract: DESIGN.md "Body model".

    model = load_body_model("assets/SMPL_NEUTRAL.pkl", "cuda")
    renderer.load_body_model(model)
    posed = model.pose(poses, shapes, R, Th)          # (F, 72), (10,) or (F, 10), (3, 3) or (F, 3, 3), (3,) or (F, 3)
    out = renderer.render(posed.tp_input(f), ...)

There is no CPU path: posing needs device tensors and the HIP library.
"""
import pickle

import numpy as np
import torch

from . import _lib

MODEL_KEYS = ('v_template', 'shapedirs', 'J_regressor', 'kintree_table', 'f', 'weights', 'posedirs')   # SMPL_to_tensor's (renderer.py:343-352)
MAX_JOINTS, MAX_SHAPES = 64, 16


def _read(src):
    if isinstance(src, dict):
        return dict(src)
    path = str(src)
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=True) as z:
            arrays = {k: z[k] for k in z.files}
        return {k: (a.item() if a.dtype == object and a.shape == () else a) for k, a in arrays.items()}      # (a pickled sparse regressor)
    try:
        with open(path, "rb") as f:          # read_pickle (renderer.py:333-337)
            u = pickle._Unpickler(f)
            u.encoding = "latin1"
            return dict(u.load())
    except ModuleNotFoundError as e:
        if "chumpy" in str(e):
            raise ImportError(f"{path} holds chumpy arrays and needs the `chumpy` package to unpickle; install it, or convert the file "
                              "to plain numpy arrays once (np.array of every entry) and load that") from e
        raise


def _dense(a):
    return np.asarray(a.toarray() if hasattr(a, "toarray") else a)


def _parents(kintree):
    """Column of every joint's parent (smpl_numpy.py:33-34); the root's entry - 4294967295 in the official files - is not read."""
    kt = np.asarray(kintree).astype(np.int64)
    col = {int(kt[1, i]): i for i in range(kt.shape[1])}
    parents = [-1]
    for i in range(1, kt.shape[1]):
        p = col.get(int(kt[0, i]), -1)
        if not 0 <= p < i:
            raise ValueError(f"kintree_table: the parent of joint {i} is {int(kt[0, i])}, which does not come before it "
                             "(the kinematic chain is walked in joint order)")
        parents.append(p)
    return parents


def load_body_model(src, device=None):
    """src: a dict, an .npz or a pickle with the SMPL keys (J_regressor may be a scipy sparse matrix) -> BodyModel on `device`."""
    raw = _read(src)
    for k in MODEL_KEYS:
        if k not in raw:
            raise KeyError(k)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    as_np = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else _dense(v)  # noqa: E731
    tensors = {}
    for k in MODEL_KEYS:                     # SMPL_to_tensor: float32, the two index tables as long
        a = np.array(as_np(raw[k])).astype(float)
        tensors[k] = torch.tensor(a, dtype=torch.long if k in ('kintree_table', 'f') else torch.float32, device=device)
    return BodyModel(tensors, _parents(as_np(raw['kintree_table'])))


class BodyModel:
    """`.tensors`: the fp32 device tensors under the SMPL_to_tensor keys (what Renderer.SMPL_NEUTRAL holds); `.parents`; the packed
    buffers of hl_body_pack, made at the first pose() and kept."""

    def __init__(self, tensors, parents):
        t = tensors
        V, J = t['weights'].shape
        if not 2 <= J <= MAX_JOINTS:
            raise ValueError(f"body model with {J} joints: the kernels take 2 .. {MAX_JOINTS}")
        if tuple(t['v_template'].shape) != (V, 3) or tuple(t['posedirs'].shape) != (V, 3, 9 * (J - 1)) or \
                tuple(t['J_regressor'].shape) != (J, V) or tuple(t['shapedirs'].shape[:2]) != (V, 3) or len(parents) != J:
            raise ValueError("body model: shapes do not fit together (v_template (V,3), shapedirs (V,3,S), posedirs (V,3,9(J-1)), "
                             "J_regressor (J,V), weights (V,J), kintree_table (2,J))")
        self.tensors = tensors
        self.parents = list(parents)
        self.V, self.J = int(V), int(J)
        self.Sp = min(int(t['shapedirs'].shape[2]), MAX_SHAPES)
        self.device = t['v_template'].device
        self.packed = None
        self._parents_dev = None
        self._big = None

    # ---- packing ---------------------------------------------------------------------------------
    def _need_device(self, what):
        if self.device.type != "cuda":
            raise RuntimeError(f"{what} needs the body model on a CUDA(HIP) device; there is no CPU path")

    def _pack(self):
        if self.packed is None:
            self._need_device("BodyModel.pose")
            L, t = _lib.lib(), self.tensors
            c = {k: t[k].contiguous() for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights')}
            buf = torch.empty(L.hl_body_packed_bytes(self.V, self.J, self.Sp) // 4, dtype=torch.float32, device=self.device)
            with _lib.on(self.device):
                _lib.check(L.hl_body_pack(_lib.ptr(c['v_template']), _lib.ptr(c['shapedirs']), int(c['shapedirs'].shape[2]),
                                          _lib.ptr(c['posedirs']), _lib.ptr(c['J_regressor']), _lib.ptr(c['weights']), self.V, self.J, self.Sp,
                                          _lib.ptr(buf), _lib.stream_ptr(self.device)), "hl_body_pack")
            self._parents_dev = torch.tensor(self.parents, dtype=torch.int32, device=self.device)
            self.packed = buf
        return self.packed

    # ---- the big pose ----------------------------------------------------------------------------
    def big_pose_params(self):
        """SynBodyView_datasets.py:185-194 for smpl_type 'smpl' (float32 numpy, like the reference)."""
        if self.J != 24:
            raise NotImplementedError("big_pose_params: the reference's big pose is defined for the 24-joint SMPL model")
        p = {'R': np.eye(3).astype(np.float32), 'Th': np.zeros((1, 3)).astype(np.float32),
             'shapes': np.zeros((1, 10)).astype(np.float32), 'poses': np.zeros((1, 72)).astype(np.float32)}
        p['poses'][0, 5] = 45 / 180 * np.array(np.pi)
        p['poses'][0, 8] = -45 / 180 * np.array(np.pi)
        p['poses'][0, 23] = -30 / 180 * np.array(np.pi)
        p['poses'][0, 26] = 30 / 180 * np.array(np.pi)
        return p

    def big_pose(self):
        """The posed big-pose body (cached): a PosedBody of one frame with `t_vertices` (V,3), `t_world_bounds` (2,3)
        (SynBodyView_datasets.py:93-101) and `rows` (V,16), the big-pose columns of every later table."""
        if self._big is None:
            bp = self.big_pose_params()
            S = min(self.Sp, bp['shapes'].shape[1])
            posed = self._pose(torch.from_numpy(bp['poses']).to(self.device), torch.zeros((S,), device=self.device), bp['R'], bp['Th'],
                               big=None)
            posed.t_vertices, posed.t_world_bounds = posed.vertices[0], posed.world_bounds[0]
            posed.t_params = {'poses': posed.poses, 'shapes': torch.zeros((1, bp['shapes'].shape[1]), device=self.device),
                              'R': posed.rt[0, :9].view(1, 3, 3), 'Th': posed.rt[0, 9:].view(1, 1, 3)}
            self._big = posed
        return self._big

    # ---- posing ----------------------------------------------------------------------------------
    def pose(self, poses, shapes, R=None, Th=None, y_margin=0.05):
        """poses (F,3J) or (3J,), shapes (S,) or (F,S): device tensors.  R (3,3) or (F,3,3), Th (3,) or (F,3): host arrays (enqueue-only)
        or device tensors (one read back here: the deform kernels take them from the host).  Returns a PosedBody of F frames.
        `y_margin`: what world_bounds adds on y beyond the 0.05 of every axis - 0.05 for SynBody, 0.1 for TightCap (TightCap_dataset.py:165-168)."""
        self._need_device("BodyModel.pose")
        return self._pose(poses, shapes, R, Th, big=self.big_pose(), y_margin=y_margin)

    def _dev(self, t, what):
        if not torch.is_tensor(t):
            t = torch.as_tensor(np.asarray(t, dtype=np.float32))
            return t.to(self.device, non_blocking=True)
        if not t.is_cuda:
            raise RuntimeError(f"BodyModel.pose: `{what}` is a CPU tensor; there is no CPU path (move it to the model's device)")
        return t.detach().to(device=self.device, dtype=torch.float32)

    def _pose(self, poses, shapes, R, Th, big, y_margin=0.05):
        self._need_device("BodyModel.pose")
        for name, t in (("poses", poses), ("shapes", shapes), ("R", R), ("Th", Th)):
            if torch.is_tensor(t) and not t.is_cuda:
                raise RuntimeError(f"BodyModel.pose: `{name}` is a CPU tensor; there is no CPU path (move it to the model's device)")
        L, J, V = _lib.lib(), self.J, self.V
        poses = self._dev(poses, "poses").reshape(-1, 3 * J).contiguous()
        F = int(poses.shape[0])
        shapes = self._dev(shapes, "shapes")
        S = int(shapes.shape[-1])
        if not 1 <= S <= self.Sp:
            raise ValueError(f"BodyModel.pose: {S} shape coefficients; this model takes 1 .. {self.Sp}")
        shapes = shapes.reshape(-1, S).contiguous()
        if shapes.shape[0] not in (1, F):
            raise ValueError(f"BodyModel.pose: shapes for {shapes.shape[0]} frames, poses for {F}")
        host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)  # noqa: E731
        Rh = np.ascontiguousarray(host(np.eye(3) if R is None else R), dtype=np.float32).reshape(-1, 3, 3)
        Thh = np.ascontiguousarray(host(np.zeros(3) if Th is None else Th), dtype=np.float32).reshape(-1, 3)
        if Rh.shape[0] not in (1, F) or Thh.shape[0] not in (1, F):
            raise ValueError(f"BodyModel.pose: R for {Rh.shape[0]} frames, Th for {Thh.shape[0]}, poses for {F}")
        n_rt = max(Rh.shape[0], Thh.shape[0])
        Rh = np.array(np.broadcast_to(Rh, (n_rt, 3, 3)), dtype=np.float32)
        Thh = np.array(np.broadcast_to(Thh, (n_rt, 3)), dtype=np.float32)
        rt_host = torch.empty((n_rt, 12), dtype=torch.float32, pin_memory=True)      # (pinned: the upload below only enqueues)
        rt_host[:, :9] = torch.from_numpy(Rh.reshape(n_rt, 9))
        rt_host[:, 9:] = torch.from_numpy(Thh)
        packed = self._pack()
        dev = self.device
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        with _lib.on(dev):
            rt = rt_host.to(dev, non_blocking=True)
            vertices, joints, bounds = new(F, V, 3), new(F, J, 3), new(F, 2, 3)
            verts4 = new(F, V, 4)
            table = new(F, V, 36) if big is not None else None
            rows = new(F, V, 16) if big is None else None
            ws = new(L.hl_body_pose_workspace_bytes(J, F) // 4)
            # (hl_body_pose with the margins of the bounds spelled out: 0.05f, 0.05f is what that call passes)
            _lib.check(L.hl_pose_body_margins(_lib.ptr(packed), _lib.ptr(self._parents_dev, torch.int32), V, J, self.Sp, S, F, _lib.ptr(poses),
                                              _lib.ptr(shapes), S if shapes.shape[0] == F and F > 1 else 0, _lib.ptr(rt), 12 if n_rt > 1 else 0,
                                              _lib.ptr(big.rows[0]) if big is not None else None, _lib.ptr(vertices), _lib.ptr(joints),
                                              _lib.ptr(bounds), _lib.ptr(verts4), _lib.ptr(table), _lib.ptr(rows), _lib.ptr(ws), ws.numel() * 4,
                                              0.05, float(y_margin), _lib.stream_ptr(dev)), "hl_pose_body_margins")
        posed = PosedBody()
        posed.model, posed.big, posed.F = self, big, F
        posed.vertices, posed.joints, posed.world_bounds, posed.verts4, posed.table, posed.rows = vertices, joints, bounds, verts4, table, rows
        posed.A, posed.pose_features = ws[:F * J * 16].view(F, J, 4, 4), ws[F * J * 16:].view(F, 9 * (J - 1))
        posed.R, posed.Th, posed.rt = Rh, Thh, rt
        posed.poses, posed.shapes = poses, shapes
        return posed


class PosedBody:
    """F posed frames.  Device tensors: vertices (F,V,3), joints (F,J,3), world_bounds (F,2,3), verts4 (F,V,4), table (F,V,36), A
    (F,J,4,4), pose_features (F,9(J-1)), poses (F,3J), shapes (1 or F,S), rt (1 or F,12) = R | Th.  Host float32 arrays: R (1 or F,3,3), Th (1 or F,3)."""

    def _rt(self, f):
        return self.R[f if self.R.shape[0] > 1 else 0], self.Th[f if self.Th.shape[0] > 1 else 0]

    def params(self, f=0):
        """Frame f's 'params' as the reference's dataset batches them: poses (1,3J), shapes (1,S), R (1,3,3), Th (1,1,3)."""
        rt = self.rt[f if self.rt.shape[0] > 1 else 0]      # (the device copy pose() uploaded: nothing moves here)
        return {'poses': self.poses[f:f + 1], 'shapes': self.shapes[f:f + 1] if self.shapes.shape[0] > 1 else self.shapes,
                'R': rt[:9].view(1, 3, 3), 'Th': rt[9:].view(1, 1, 3)}

    def deform(self, f=0):
        """(verts4 (V,4), table (V,36), R host (3,3), Th host (3,)) of frame f: what deform_tables returns."""
        Rf, Tf = self._rt(f)
        return (self.verts4[f], self.table[f], np.ascontiguousarray(Rf), np.ascontiguousarray(Tf))

    def tp_input(self, f=0):
        """The pieces of tp_input the reference's dataset makes for one posed frame (SynBodyView_datasets.py:300-306), batch 1, plus
        'deform': frame f's prebuilt tables, which the renderer uses instead of building them (and fingerprinting the vertices)."""
        if self.big is None:
            raise RuntimeError("tp_input: this is the big-pose body itself")
        return {'params': self.params(f), 't_params': dict(self.big.t_params), 'vertices': self.vertices[f:f + 1], 'world_bounds': self.world_bounds[f:f + 1],
                't_world_bounds': self.big.t_world_bounds[None], 'deform': self.deform(f)}

    def bounds_host(self):
        """All frames' world bounds (F,2,3) as one host array - one copy, for camera_rays."""
        return self.world_bounds.cpu().numpy()
