"""The body model on the device: loading an SMPL-style asset and posing it with the hl_body_* / hl_smplx_* kernels (csrc/hl_body.hip).

The reference poses the body in its dataset code with numpy (smpl/smpl_numpy.py, SynBodyView_datasets.py:141-194) and rebuilds the
per-point deformation inputs with stock PyTorch ops.  Here one call poses a frame or a whole sequence: posed vertices, joints and
world bounds as `prepare_input` returns them, plus the (verts4, table) pair hl_deform_points / hl_deform_rays consume, so that a
renderer handed `tp_input['deform']` runs no torch op chain and reads nothing back per view.  Contract: DESIGN.md "Body model".

    model = load_body_model("assets/SMPL_NEUTRAL.pkl", "cuda")
    renderer.load_body_model(model)
    posed = model.pose(poses, shapes, R, Th)          # (F, 72), (10,) or (F, 10), (3, 3) or (F, 3, 3), (3,) or (F, 3)
    out = renderer.render(posed.tp_input(f), ...)

SMPL-X, which the reference's SynBody flows use by default, has a loader of its own and runs the same kernels with its additions
compiled in; it returns the same PosedBody:

    model = load_smplx_model("assets/models/smplx", "cuda", gender="female")
    posed = model.pose_dict(params)                   # the keys of <subject>/smplx.npz: global_orient, body_pose, betas, expression, ...

There is no CPU path: posing needs device tensors and the HIP library.
"""
import os
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


def _as_np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else _dense(v)


def _model_tensors(raw, device, posedirs_2d=False):
    """SMPL_to_tensor on `device`: MODEL_KEYS as float32, the two index tables as long -> (tensors, parents).  `posedirs_2d`: a (3V,P)
    posedirs, as the SMPL-X files store it, becomes (V,3,P)."""
    tensors = {}
    for k in MODEL_KEYS:
        a = np.array(_as_np(raw[k])).astype(float)
        if posedirs_2d and k == 'posedirs' and a.ndim == 2:
            a = a.reshape(a.shape[0] // 3, 3, -1)
        tensors[k] = torch.tensor(a, dtype=torch.long if k in ('kintree_table', 'f') else torch.float32, device=device)
    return tensors, _parents(_as_np(raw['kintree_table']))


def load_body_model(src, device=None):
    """src: a dict, an .npz or a pickle with the SMPL keys (J_regressor may be a scipy sparse matrix) -> BodyModel on `device`."""
    raw = _read(src)
    for k in MODEL_KEYS:
        if k not in raw:
            raise KeyError(k)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return BodyModel(*_model_tensors(raw, device))


class _DeviceModel:
    """What BodyModel and SmplxModel share: the check of the model's arrays, the packed buffers (made at the first pose and kept), the
    staging of a call's inputs and outputs, and the PosedBody.  A subclass names itself (`NAME`, `LABEL`), packs (`_pack_into`) and
    hands `_run` the arguments of its pose entry point."""

    def __init__(self, tensors, parents):
        t = tensors
        V, J = t['weights'].shape
        if tuple(t['v_template'].shape) != (V, 3) or tuple(t['posedirs'].shape) != (V, 3, 9 * (J - 1)) or \
                tuple(t['J_regressor'].shape) != (J, V) or tuple(t['shapedirs'].shape[:2]) != (V, 3) or len(parents) != J:
            raise ValueError(f"{self.LABEL}: shapes do not fit together (v_template (V,3), shapedirs (V,3,S), posedirs (V,3,9(J-1)), "
                             "J_regressor (J,V), weights (V,J), kintree_table (2,J))")
        self.tensors, self.parents = tensors, list(parents)
        self.V, self.J = int(V), int(J)
        self.device = t['v_template'].device
        self.packed = None
        self._parents_dev = None

    def _need_device(self):
        if self.device.type != "cuda":
            raise RuntimeError(f"{self.NAME}.pose needs the body model on a CUDA(HIP) device; there is no CPU path")

    def _pack(self):
        if self.packed is None:
            self._need_device()
            c = {k: self.tensors[k].contiguous() for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights')}
            packed = self._pack_into(_lib.lib(), c)
            self._parents_dev = torch.tensor(self.parents, dtype=torch.int32, device=self.device)
            self.packed = packed
        return self.packed

    def _dev(self, t, what):
        if not torch.is_tensor(t):
            return torch.as_tensor(np.asarray(t, dtype=np.float32)).to(self.device, non_blocking=True)
        if not t.is_cuda:
            raise RuntimeError(f"{self.NAME}.pose: `{what}` is a CPU tensor; there is no CPU path (move it to the model's device)")
        return t.detach().to(device=self.device, dtype=torch.float32)

    def _run(self, entry, model_args, ws_bytes, ws_joint_floats, F, poses, shapes, R, Th, big, y_margin, forward_rows=False):
        """One call of the pose entry point `entry`: `model_args` are its arguments between J and rt, `ws_bytes` names its workspace
        query; the workspace is A (F,J,16) | ... | the pose features (F,P), `ws_joint_floats` per joint before the features.  R, Th:
        host arrays or tensors, one or F of each (None: I, 0).  `forward_rows`: also write the (F,V,16) forward rows (what the big pose always
        gets).  Returns the PosedBody of the F frames."""
        L, J, V, dev = _lib.lib(), self.J, self.V, self.device
        host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)  # noqa: E731
        Rh = np.ascontiguousarray(host(np.eye(3) if R is None else R), dtype=np.float32).reshape(-1, 3, 3)
        Thh = np.ascontiguousarray(host(np.zeros(3) if Th is None else Th), dtype=np.float32).reshape(-1, 3)
        if Rh.shape[0] not in (1, F) or Thh.shape[0] not in (1, F):
            raise ValueError(f"{self.NAME}.pose: R for {Rh.shape[0]} frames, Th for {Thh.shape[0]}, poses for {F}")
        n_rt = max(Rh.shape[0], Thh.shape[0])
        Rh = np.array(np.broadcast_to(Rh, (n_rt, 3, 3)), dtype=np.float32)
        Thh = np.array(np.broadcast_to(Thh, (n_rt, 3)), dtype=np.float32)
        rt_host = torch.empty((n_rt, 12), dtype=torch.float32, pin_memory=True)      # (pinned: the upload below only enqueues)
        rt_host[:, :9] = torch.from_numpy(Rh.reshape(n_rt, 9))
        rt_host[:, 9:] = torch.from_numpy(Thh)
        packed = self._pack()
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        with _lib.on(dev):
            rt = rt_host.to(dev, non_blocking=True)
            vertices, joints, bounds, verts4 = new(F, V, 3), new(F, J, 3), new(F, 2, 3), new(F, V, 4)
            table = new(F, V, 36) if big is not None else None
            rows = new(F, V, 16) if big is None or forward_rows else None
            ws = new(getattr(L, ws_bytes)(J, F) // 4)
            _lib.check(getattr(L, entry)(_lib.ptr(packed), _lib.ptr(self._parents_dev, torch.int32), V, J, *model_args, _lib.ptr(rt),
                                         12 if n_rt > 1 else 0, _lib.ptr(big.rows[0]) if big is not None else None, _lib.ptr(vertices),
                                         _lib.ptr(joints), _lib.ptr(bounds), _lib.ptr(verts4), _lib.ptr(table), _lib.ptr(rows), _lib.ptr(ws),
                                         ws.numel() * 4, 0.05, float(y_margin), _lib.stream_ptr(dev)), entry)
        posed = PosedBody()
        posed.model, posed.big, posed.F = self, big, F
        posed.vertices, posed.joints, posed.world_bounds, posed.verts4, posed.table, posed.rows = vertices, joints, bounds, verts4, table, rows
        posed.A, posed.pose_features = ws[:F * J * 16].view(F, J, 4, 4), ws[F * J * ws_joint_floats:].view(F, 9 * (J - 1))
        posed.R, posed.Th, posed.rt = Rh, Thh, rt
        posed.poses, posed.shapes = poses, shapes
        return posed


class BodyModel(_DeviceModel):
    """`.tensors`: the fp32 device tensors under the SMPL_to_tensor keys (what Renderer.SMPL_NEUTRAL holds); `.parents`; the packed
    buffers of hl_body_pack, made at the first pose() and kept."""
    NAME, LABEL = "BodyModel", "body model"

    def __init__(self, tensors, parents):
        J = tensors['weights'].shape[1]
        if not 2 <= J <= MAX_JOINTS:
            raise ValueError(f"body model with {J} joints: the kernels take 2 .. {MAX_JOINTS}")
        super().__init__(tensors, parents)
        self.Sp = min(int(tensors['shapedirs'].shape[2]), MAX_SHAPES)
        self._big = None

    def _pack_into(self, L, c):
        buf = torch.empty(L.hl_body_packed_bytes(self.V, self.J, self.Sp) // 4, dtype=torch.float32, device=self.device)
        with _lib.on(self.device):
            _lib.check(L.hl_body_pack(_lib.ptr(c['v_template']), _lib.ptr(c['shapedirs']), int(c['shapedirs'].shape[2]),
                                      _lib.ptr(c['posedirs']), _lib.ptr(c['J_regressor']), _lib.ptr(c['weights']), self.V, self.J, self.Sp,
                                      _lib.ptr(buf), _lib.stream_ptr(self.device)), "hl_body_pack")
        return buf

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
    def pose(self, poses, shapes, R=None, Th=None, y_margin=0.05, forward_rows=False):
        """poses (F,3J) or (3J,), shapes (S,) or (F,S): device tensors.  R (3,3) or (F,3,3), Th (3,) or (F,3): host arrays (enqueue-only)
        or device tensors (one read back here: the deform kernels take them from the host).  Returns a PosedBody of F frames.
        `y_margin`: what world_bounds adds on y beyond the 0.05 of every axis - 0.05 for SynBody, 0.1 for TightCap (TightCap_dataset.py:165-168).
        `forward_rows`: also keep `.rows` (F,V,16), the blended R[9] t[3] pose_off[3] pad[1] of every vertex, which NeRF/animate.py binds
        an extracted mesh to and reposes it from."""
        self._need_device()
        return self._pose(poses, shapes, R, Th, big=self.big_pose(), y_margin=y_margin, forward_rows=forward_rows)

    def _pose(self, poses, shapes, R, Th, big, y_margin=0.05, forward_rows=False):
        self._need_device()
        for name, t in (("poses", poses), ("shapes", shapes), ("R", R), ("Th", Th)):
            if torch.is_tensor(t) and not t.is_cuda:
                raise RuntimeError(f"BodyModel.pose: `{name}` is a CPU tensor; there is no CPU path (move it to the model's device)")
        poses = self._dev(poses, "poses").reshape(-1, 3 * self.J).contiguous()
        F = int(poses.shape[0])
        shapes = self._dev(shapes, "shapes")
        S = int(shapes.shape[-1])
        if not 1 <= S <= self.Sp:
            raise ValueError(f"BodyModel.pose: {S} shape coefficients; this model takes 1 .. {self.Sp}")
        shapes = shapes.reshape(-1, S).contiguous()
        if shapes.shape[0] not in (1, F):
            raise ValueError(f"BodyModel.pose: shapes for {shapes.shape[0]} frames, poses for {F}")
        # (hl_body_pose with the margins of the bounds spelled out: 0.05f, 0.05f is what that call passes)
        args = (self.Sp, S, F, _lib.ptr(poses), _lib.ptr(shapes), S if shapes.shape[0] == F and F > 1 else 0)
        return self._run("hl_pose_body_margins", args, "hl_body_pose_workspace_bytes", 16, F, poses, shapes, R, Th, big, y_margin, forward_rows)


class PosedBody:
    """F posed frames.  Device tensors: vertices (F,V,3), joints (F,J,3), world_bounds (F,2,3), verts4 (F,V,4), table (F,V,36), A
    (F,J,4,4), pose_features (F,9(J-1)), poses (F,3J), shapes (1 or F,S), rt (1 or F,12) = R | Th, rows (F,V,16) when posed with forward_rows=True
    (None otherwise).  Host float32 arrays: R (1 or F,3,3), Th (1 or F,3)."""

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


# ---- SMPL-X -------------------------------------------------------------------------------------------------------------------------
SMPLX_KEYS = MODEL_KEYS + ('hands_meanl', 'hands_meanr')                 # what the reference's SMPLX reads for use_pca=False, without landmarks
SMPLX_PARTS = (('global_orient', 1), ('body_pose', 21), ('jaw_pose', 1), ('leye_pose', 1), ('reye_pose', 1), ('left_hand_pose', 15),
               ('right_hand_pose', 15))                                   # full_pose, in this order (body_models.py:1215-1222)
SMPLX_MAX_COEFFS = 32
SHAPE_SPACE_DIM, EXPRESSION_SPACE_DIM = 300, 100


def load_smplx_model(src, device=None, num_betas=10, num_expression_coeffs=10, flat_hand_mean=True, use_pca=False, gender='neutral'):
    """src: a dict, an .npz or a pickle with the SMPL-X keys, or a directory, which resolves to SMPLX_{GENDER}.npz as the reference's
    SMPLX does (body_models.py:975-979) -> SmplxModel on `device`.  The expression directions are columns [300, 300 + n) of a file with
    at least 400 shape columns and [10, 10 + min(n, 10)) otherwise (:1057-1077)."""
    if use_pca:
        raise NotImplementedError("load_smplx_model: use_pca=True (PCA hand poses) is not restated; no shipped configuration uses it")
    if not isinstance(src, dict) and os.path.isdir(str(src)):
        src = os.path.join(str(src), f"SMPLX_{gender.upper()}.npz")
    raw = _read(src)
    for k in SMPLX_KEYS:
        if k not in raw:
            raise KeyError(k)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    tensors, parents = _model_tensors(raw, device, posedirs_2d=True)
    cols = int(tensors['shapedirs'].shape[2])
    if cols < SHAPE_SPACE_DIM + EXPRESSION_SPACE_DIM:
        num_betas, e0, num_expr = min(int(num_betas), 10), 10, min(int(num_expression_coeffs), 10)
    else:
        num_betas, e0, num_expr = min(int(num_betas), SHAPE_SPACE_DIM), SHAPE_SPACE_DIM, min(int(num_expression_coeffs), EXPRESSION_SPACE_DIM)
    pose_mean = np.zeros(3 * sum(n for _, n in SMPLX_PARTS), dtype=np.float32)
    if not flat_hand_mean:
        pose_mean[-90:-45] = np.asarray(_as_np(raw['hands_meanl']), dtype=np.float32).reshape(-1)
        pose_mean[-45:] = np.asarray(_as_np(raw['hands_meanr']), dtype=np.float32).reshape(-1)
    return SmplxModel(tensors, parents, num_betas, e0, num_expr, torch.from_numpy(pose_mean).to(device))


def load_smplx_models(model_dir, device=None, genders=('male', 'female', 'neutral'), **kw):
    """{gender: SmplxModel} of every SMPLX_{GENDER}.npz `model_dir` holds - what the reference's SynBody datasets keep (SynBody_dataset.py:
    84-99) and load_view_store(..., smpl_type='smplx') takes.  `kw`: load_smplx_model's."""
    found = {g: load_smplx_model(model_dir, device, gender=g, **kw) for g in genders if os.path.exists(os.path.join(str(model_dir), f"SMPLX_{g.upper()}.npz"))}
    if not found:
        raise FileNotFoundError(f"{model_dir}: none of " + ", ".join(f"SMPLX_{g.upper()}.npz" for g in genders))
    return found


class SmplxModel(_DeviceModel):
    """An SMPL-X body on the device (csrc/hl_body.hip).  `.tensors`: the fp32 device tensors under the SMPL_to_tensor keys,
    shapedirs with every column of the file (what Renderer.SMPL_NEUTRAL holds for smpl_type 'smplx'); `.parents`; `.num_betas`,
    `.expr_start`, `.num_expr`: the columns of shapedirs that shape the body; `.pose_mean` (165,)."""
    NAME, LABEL = "SmplxModel", "SMPL-X model"

    def __init__(self, tensors, parents, num_betas, expr_start, num_expr, pose_mean):
        J = tensors['weights'].shape[1]
        if J != sum(n for _, n in SMPLX_PARTS):
            raise ValueError(f"SMPL-X model with {J} joints: the full pose has {sum(n for _, n in SMPLX_PARTS)}")
        super().__init__(tensors, parents)
        cols = int(tensors['shapedirs'].shape[2])
        S = num_betas + num_expr
        if not (1 <= S <= SMPLX_MAX_COEFFS and num_betas <= expr_start and expr_start + num_expr <= cols):
            raise ValueError(f"SMPL-X model: {num_betas} betas and {num_expr} expression coefficients from column {expr_start} of {cols}; "
                             f"the kernels take 1 .. {SMPLX_MAX_COEFFS} coefficients in all")
        self.S = int(S)
        self.num_betas, self.expr_start, self.num_expr = int(num_betas), int(expr_start), int(num_expr)
        self.two_sets = int(num_expr > 0 and expr_start != num_betas)
        self.pose_mean = pose_mean
        self._big = {}

    def _pack_into(self, L, c):
        buf = torch.empty(L.hl_smplx_packed_bytes(self.V, self.J, self.S, self.two_sets) // 4, dtype=torch.float32, device=self.device)
        with _lib.on(self.device):
            _lib.check(L.hl_smplx_pack(_lib.ptr(c['v_template']), _lib.ptr(c['shapedirs']), int(c['shapedirs'].shape[2]), self.num_betas,
                                       self.expr_start, self.num_expr, _lib.ptr(c['posedirs']), _lib.ptr(c['J_regressor']),
                                       _lib.ptr(c['weights']), self.V, self.J, _lib.ptr(buf), _lib.stream_ptr(self.device)), "hl_smplx_pack")
        return buf

    # ---- the big pose ----------------------------------------------------------------------------
    def big_pose_params(self, global_orient=None):
        """The reference's big pose for smpl_type 'smplx' (float32 numpy).  Its two twins differ in the global orientation: zero in
        recon_NeRF/lib/SynBody_dataset.py:207-224 (the default here), [-3.1416, 0, 0] in human_diffusion/SynBodyView_datasets.py:196-212."""
        z = lambda n: np.zeros((1, n)).astype(np.float32)  # noqa: E731
        p = {'R': np.eye(3).astype(np.float32), 'Th': z(3), 'global_orient': z(3), 'betas': z(self.num_betas), 'body_pose': z(63), 'jaw_pose': z(3),
             'left_hand_pose': z(45), 'right_hand_pose': z(45), 'leye_pose': z(3), 'reye_pose': z(3), 'expression': z(self.num_expr), 'transl': z(3)}
        if global_orient is not None:
            p['global_orient'] = np.asarray(global_orient, dtype=np.float32).reshape(1, 3)
        p['body_pose'][0, 2] = 45 / 180 * np.array(np.pi)
        p['body_pose'][0, 5] = -45 / 180 * np.array(np.pi)
        p['body_pose'][0, 20] = -30 / 180 * np.array(np.pi)
        p['body_pose'][0, 23] = 30 / 180 * np.array(np.pi)
        return p

    def big_pose(self, global_orient=None):
        """The posed big-pose body, cached per global orientation: a PosedBody of one frame with `t_vertices`, `t_world_bounds`, `t_params`
        and `rows` (V,16), the big-pose columns of every later table."""
        key = tuple(np.zeros(3, dtype=np.float32) if global_orient is None else np.asarray(global_orient, dtype=np.float32).reshape(3))
        if key not in self._big:
            bp = self.big_pose_params(global_orient)
            posed = self._pose({k: torch.from_numpy(bp[k]).to(self.device) for k, _ in SMPLX_PARTS}, torch.from_numpy(bp['betas']).to(self.device),
                               torch.from_numpy(bp['expression']).to(self.device), None, bp['R'], bp['Th'], big=None)
            posed.t_vertices, posed.t_world_bounds = posed.vertices[0], posed.world_bounds[0]
            posed.t_params = {'poses': posed.poses, 'shapes': posed.shapes, 'R': posed.rt[0, :9].view(1, 3, 3), 'Th': posed.rt[0, 9:].view(1, 1, 3)}
            self._big[key] = posed
        return self._big[key]

    # ---- posing ----------------------------------------------------------------------------------
    def pose(self, global_orient, body_pose, betas, expression, jaw_pose=None, leye_pose=None, reye_pose=None, left_hand_pose=None,
             right_hand_pose=None, transl=None, R=None, Th=None, y_margin=0.05, big_global_orient=None, forward_rows=False):
        """SMPLX.forward for F frames: global_orient (F,3), body_pose (F,63), betas (nb,) / (1,nb) shared or (F,nb), expression (F,ne), the
        other parts (F,3) / (F,45) or None for zeros, transl (F,3) or None: device tensors (host arrays are uploaded).  R, Th: the dataset's
        world transform, as BodyModel.pose takes them.  `big_global_orient`: which big pose the tables' canonical columns come from.
        `forward_rows`: as BodyModel.pose (the rows are shape set 1's and, like every row, without transl)."""
        self._need_device()
        parts = {'global_orient': global_orient, 'body_pose': body_pose, 'jaw_pose': jaw_pose, 'leye_pose': leye_pose, 'reye_pose': reye_pose,
                 'left_hand_pose': left_hand_pose, 'right_hand_pose': right_hand_pose}
        return self._pose(parts, betas, expression, transl, R, Th, big=self.big_pose(big_global_orient), y_margin=y_margin, forward_rows=forward_rows)

    def pose_dict(self, d, R=None, Th=None, y_margin=0.05, big_global_orient=None, forward_rows=False):
        """pose() of a dict under the key names of a SynBody smplx.npz (missing parts are zeros; other keys are ignored).  Host tensors,
        as the dataset's prepare_smpl_params makes them, are uploaded."""
        self._need_device()
        d = {k: (v.to(self.device) if torch.is_tensor(v) and k not in ('R', 'Th') else v) for k, v in d.items()}
        return self.pose(d['global_orient'], d['body_pose'], d['betas'], d['expression'], d.get('jaw_pose'), d.get('leye_pose'), d.get('reye_pose'),
                         d.get('left_hand_pose'), d.get('right_hand_pose'), d.get('transl'), R if R is not None else d.get('R'),
                         Th if Th is not None else d.get('Th'), y_margin=y_margin, big_global_orient=big_global_orient, forward_rows=forward_rows)

    def _pose(self, parts, betas, expression, transl, R, Th, big, y_margin=0.05, forward_rows=False):
        self._need_device()
        dev = self.device
        go = self._dev(parts['global_orient'], 'global_orient').reshape(-1, 3)
        F = int(go.shape[0])
        cols = []
        for name, n in SMPLX_PARTS:
            p = parts.get(name)
            p = torch.zeros((F, 3 * n), dtype=torch.float32, device=dev) if p is None else self._dev(p, name).reshape(-1, 3 * n)
            if p.shape[0] != F:
                raise ValueError(f"SmplxModel.pose: `{name}` for {p.shape[0]} frames, global_orient for {F}")
            cols.append(p)
        poses = (torch.cat(cols, dim=1) + self.pose_mean).contiguous()                     # full_pose += pose_mean (body_models.py:1226)
        betas = self._dev(betas, 'betas').reshape(-1, self.num_betas) if self.num_betas else torch.zeros((1, 0), device=dev)
        expression = self._dev(expression, 'expression').reshape(-1, self.num_expr) if self.num_expr else torch.zeros((F, 0), device=dev)
        if betas.shape[0] not in (1, F) or expression.shape[0] != F:
            raise ValueError(f"SmplxModel.pose: betas for {betas.shape[0]} frames, expression for {expression.shape[0]}, poses for {F}")
        coef = torch.cat([betas.expand(F, -1), expression], dim=1).contiguous()             # shape_components (:1234)
        if transl is not None:
            transl = self._dev(transl, 'transl').reshape(-1, 3).contiguous()
            if transl.shape[0] != F:
                raise ValueError(f"SmplxModel.pose: transl for {transl.shape[0]} frames, poses for {F}")
        args = (self.S, self.two_sets, F, _lib.ptr(poses), _lib.ptr(coef), _lib.ptr(transl))
        posed = self._run("hl_smplx_pose", args, "hl_smplx_pose_workspace_bytes", 20, F, poses, coef, R, Th, big, y_margin, forward_rows)
        posed.transl = transl
        return posed
