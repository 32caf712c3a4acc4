"""FitLoop: the tri-plane fitting loop of recon_NeRF/run_nerf_batch.py:227-329 (and run_nerf_batch_ft.py) with its tail on HIP.

    loop = FitLoop(model, loader, lrate=5e-4, tri_plane_lrate=1e-1, lrate_decay=10, tv_loss_coef=1e-2, l1_loss_coef=5e-4,
                   use_clamp=True, n_samples=128, n_importance=128, basedir="logs", expname="fit")
    loop.run_loop()                     # or: losses = loop.step(tp_input)

One iteration (run_nerf_batch.py:236-301, restated):
  gather   x = tri_planes[instance_idx, cloth_layer_index] on the device, a LEAF tensor: the render backward leaves the batch's
           gradient in x.grad (bs x 27 x H x W); nothing ever lands on the 2.83 GB `tri_planes.grad` of a 100-subject run
  render   humanliff_amd.NeRF.render -> RenderRaysFunction (HIP forward and backward), img2mse(rgb, target) + 0.1 img2mse(mask, acc)
  reg      hl_fit_reg: the TV and L1 sums of :256-259 and their gradient added to x.grad, one pass
  MLP      the 14 decoder tensors through FusedAdamW's launch (weight decay 0, no EMA); not with ft_triplane_only
  planes   hl_fit_adam_planes: Adam over ALL of tri_planes, the gradient of a slice formed in the kernel from x.grad and the batch's
           DEVICE indices (never read by the host), then clamp_(-1, 1) when use_clamp
  lr       the two exponential schedules of :281-297, from the pre-increment global_step
The five losses stay on the device; run_loop reads their running sums every i_print steps.

Differences from the reference loop, on purpose: TV / L1 are always computed (without --tv_loss the reference stops at :262, l1_loss
undefined); the checkpoint's optimizer state is loaded back on resume (the reference writes it and leaves the load commented out,
:107), so a resumed run continues bit-identically; run_loop stops at n_iteration + 1 steps instead of at the end of that epoch; the
printed losses and time are means over the steps the window really holds (a single iteration's host time says nothing when nothing
synchronises; the first window after a resume may be short).  sign(NaN) is NaN in the regularisers' gradient: torch's l1_loss backward
goes through torch.sign, which returns 0 for NaN, so the PyTorch loop leaves a zero gradient at a NaN texel where this one leaves NaN -
a deliberate difference (a poisoned plane stays visible), not one to "fix" on either side.  One process drives one GPU: a DDP / DataParallel wrapper is unwrapped and
its gradient exchange is not used.  There is no eager fallback: a CPU module or a missing library raises.
"""
import ctypes as C
import math
import os
import time

import torch

from .. import _lib
from ..NeRF.renderer import render as _render
from ..optim import FusedAdamW
from .run_nerf_batch import _Bare

LR_LAST_STEP = 300000      # run_nerf_batch.py:281
MAX_BATCH = 64             # HL_FIT_MAX_BATCH of include/humanliff_hip.h: the kernel keeps the selecting entries in a 64-bit mask


def lr_schedule(global_step, lrate, tri_plane_lrate, lrate_decay):
    """(MLP lr, tri-plane lr) that run_nerf_batch.py:281-288 sets after the iteration whose pre-increment counter is global_step;
    past step 300 000 the reference stops updating, which leaves the values of step 300 000."""
    s = min(global_step, LR_LAST_STEP)
    return lrate * (0.1 ** (s / (lrate_decay * 600))), tri_plane_lrate * (0.5 ** (s / (lrate_decay * 60)))


def img2mse(x, y):
    return torch.mean((x - y) ** 2)


def mse2psnr(x):
    return -10.0 * math.log(x) / math.log(10.0)


def split_parameters(core):
    """create_nerf (run_nerf_batch.py:80-86): every parameter but `tri_planes`, in named_parameters() order, and tri_planes."""
    mlp = [p for n, p in core.named_parameters() if n != 'tri_planes']
    return mlp, core.tri_planes


class FitAdam(torch.optim.Optimizer):
    """torch.optim.Adam([{'params': mlp, 'lr': lrate}, {'params': [tri_planes], 'lr': tri_plane_lrate}], betas=(0.9, 0.999)) of
    create_nerf (:89) with the same param_groups and per-parameter state (`step` on the host, `exp_avg`, `exp_avg_sq`), so
    state_dict() loads into that optimizer and back.  Group 0 steps through FusedAdamW's table launch, group 1 through
    hl_fit_adam_planes, which takes the batch's gradient buffers and device indices instead of a dense .grad."""

    def __init__(self, mlp_params, tri_planes, lrate, tri_plane_lrate, betas=(0.9, 0.999), eps=1e-8):
        defaults = dict(lr=lrate, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=False)      # torch.optim.Adam's own keys
        super().__init__([{'params': list(mlp_params), 'lr': lrate}, {'params': [tri_planes], 'lr': tri_plane_lrate}], defaults)
        self._link()

    def _link(self):
        """Group 0's launch plan lives in a FusedAdamW over the same parameters that keeps its state in this optimizer's own `state`
        (weight_decay 0: AdamW's update is Adam's)."""
        g0 = self.param_groups[0]
        self._mlp = None
        if g0['params']:
            self._mlp = FusedAdamW(g0['params'], lr=g0['lr'], betas=g0['betas'], eps=g0['eps'], weight_decay=0.0)
            self._mlp.state = self.state

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():        # Adam keeps `step` on the host (not capturable); load_state_dict moves it with the parameter
            if torch.is_tensor(st.get("step")):
                st["step"] = st["step"].detach().to("cpu", torch.float32)
        self._link()

    def init_state(self):
        """Allocate the state of every parameter (zero moments, step 0), as a first step of each group would."""
        if self._mlp is not None:
            for p in self.param_groups[0]['params']:
                self._mlp._state(p)
        self.planes_state()

    def planes_state(self):
        p = self.param_groups[1]['params'][0]
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step_mlp(self):
        """Adam on every group-0 parameter that has a .grad: one hl_adamw_step launch."""
        if self._mlp is not None:
            self._mlp.param_groups[0]['lr'] = self.param_groups[0]['lr']
            self._mlp.step()

    @torch.no_grad()
    def step_planes(self, grad, instance_idx, layer_idx, clamp):
        """Adam over the whole tri_planes parameter (NI, NL, ...): grad (bs, ...) holds the batch entries' gradients, entry b belonging
        to slice (instance_idx[b], layer_idx[b]) - int64 device tensors the host never reads.  Enqueue-only."""
        grp = self.param_groups[1]
        p = grp['params'][0]
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError("FitAdam: tri_planes must be a contiguous float32 tensor on a HIP device (there is no CPU path)")
        NI, NL = p.shape[:2]
        L_ = p[0, 0].numel()
        bs = grad.shape[0]
        if not 1 <= bs <= MAX_BATCH:
            raise RuntimeError(f"FitAdam: a batch of {bs} entries; hl_fit_adam_planes takes 1 to {MAX_BATCH}")
        if grad.dtype != torch.float32 or grad.device != p.device or not grad.is_contiguous() or grad[0].numel() != L_:
            raise RuntimeError("FitAdam: the gradient buffers must be one contiguous float32 tensor (bs, ...) of tri_planes' slices")
        for t in (instance_idx, layer_idx):
            if t.dtype != torch.int64 or t.device != p.device or t.shape != (bs,) or not t.is_contiguous():
                raise RuntimeError("FitAdam: instance_idx / cloth_layer_index must be contiguous int64 device tensors of shape (bs,)")
        st = self.planes_state()
        m, v = st["exp_avg"], st["exp_avg_sq"]
        st["step"] += 1                                       # (a host tensor: no device work)
        step = float(st["step"])
        lr, (b1, b2), eps = float(grp["lr"]), grp["betas"], grp["eps"]
        bc1 = 1.0 - b1 ** step                               # the scalars in double on the host, as torch computes them
        bc2 = 1.0 - b2 ** step
        q = _lib.ptr
        with _lib.on(p.device):
            _lib.check(_lib.lib().hl_fit_adam_planes(q(p.detach()), q(m), q(v), q(grad), q(instance_idx), q(layer_idx), bs, NI, NL, L_,
                                                     1.0 - b1, b2, 1.0 - b2, bc2 ** 0.5, eps, -(lr / bc1), 1 if clamp else 0,
                                                     _lib.stream_ptr(p.device)), "hl_fit_adam_planes")


def fit_reg(planes, grad, tv_loss_coef, l1_loss_coef):
    """hl_fit_reg on the gathered plane sets (bs, 3, C, H, W) and their gradient buffer (added to in place).  Returns (tv_loss, l1_loss)
    as float32 device scalars: F.l1_loss's means of run_nerf_batch.py:256-259 over the whole batch.  Enqueue-only."""
    if not planes.is_cuda:
        raise RuntimeError("fit_reg needs HIP tensors; there is no CPU path")
    if planes.dtype != torch.float32 or grad.dtype != torch.float32 or planes.shape != grad.shape or planes.dim() < 3 \
            or not planes.is_contiguous() or not grad.is_contiguous() or grad.device != planes.device:
        raise RuntimeError("fit_reg: planes and grad must be contiguous float32 tensors of one shape (..., H, W) on one device")
    H, W = planes.shape[-2:]
    if H < 2 or W < 2:
        raise RuntimeError(f"fit_reg: images of {H} x {W}; the total variation needs H, W >= 2")
    n = planes.numel()
    nplanes = n // (H * W)
    n_x, n_y = nplanes * (H - 1) * W, nplanes * H * (W - 1)
    L = _lib.lib()
    dev = planes.device
    scratch = torch.empty(L.hl_fit_reg_scratch_bytes(nplanes, H, W) // 8, dtype=torch.float64, device=dev)
    sums = torch.empty(3, dtype=torch.float64, device=dev)
    with _lib.on(dev):
        _lib.check(L.hl_fit_reg(_lib.ptr(planes), _lib.ptr(grad), nplanes, H, W, tv_loss_coef / n_x, tv_loss_coef / n_y, l1_loss_coef / n,
                                C.c_void_p(sums.data_ptr()), C.c_void_p(scratch.data_ptr()), scratch.numel() * 8, _lib.stream_ptr(dev)),
                   "hl_fit_reg")
    return (sums[0] / n_x + sums[1] / n_y).float(), (sums[2] / n).float()      # (fp64 until the last rounding)


def checkpoint_dict(core, optimizer, global_step):
    """The reference's checkpoint (:325-329)."""
    return {'global_step': global_step, 'network_fn_state_dict': core.state_dict(), 'optimizer_state_dict': optimizer.state_dict()}


class FitLoop:
    def __init__(self, renderer, data, *, lrate=5e-4, tri_plane_lrate=1e-3, lrate_decay=250, tv_loss_coef=5e-4, l1_loss_coef=2e-4,
                 use_clamp=False, n_samples=64, n_importance=0, perturb=1., chunk=1024 * 64, ft_triplane_only=False, n_iteration=50000,
                 i_print=100, i_weights=10000, basedir='./logs/', expname=None, ft_path=None, no_reload=False):
        core = renderer.module if hasattr(renderer, "module") else renderer
        if not core.tri_planes.is_cuda or not all(p.is_cuda for p in core.parameters()):
            raise RuntimeError("FitLoop needs the Renderer on a HIP device (call .to('cuda')); humanliff_amd has no CPU path")
        _lib.lib()
        self.core, self.data = core, data
        self.lrate, self.tri_plane_lrate, self.lrate_decay = lrate, tri_plane_lrate, lrate_decay
        self.tv_loss_coef, self.l1_loss_coef, self.use_clamp = tv_loss_coef, l1_loss_coef, use_clamp
        self.n_samples, self.n_importance, self.perturb, self.chunk = n_samples, n_importance, perturb, chunk
        self.ft_triplane_only, self.n_iteration, self.i_print, self.i_weights = ft_triplane_only, n_iteration, i_print, i_weights
        self.logdir = os.path.join(basedir, expname) if expname is not None else None
        mlp, planes = split_parameters(core)
        if ft_triplane_only:                                  # run_nerf_batch_ft.py:124-129
            for p in mlp:
                p.requires_grad_(False)
            planes.requires_grad_(True)
        self.optimizer = FitAdam(mlp, planes, lrate, tri_plane_lrate)
        self.global_step = 0
        self.tail_event = None              # a torch.cuda.Event to record between the render backward and the tail (scripts/fit_loop_time.py)
        core.train()
        if self.logdir is not None and not no_reload:         # create_nerf, :95-112: the named file, else the newest .tar of the run
            if ft_path is not None and ft_path != 'None':
                ckpts = [os.path.join(self.logdir, ft_path)]
            elif os.path.isdir(self.logdir):
                ckpts = [os.path.join(self.logdir, f) for f in sorted(os.listdir(self.logdir)) if '.tar' in f]
            else:
                ckpts = []
            if ckpts:
                self.load_checkpoint(ckpts[-1])

    # ---- checkpoints (the reference's layout, :325-329) ------------------------------------------------------------------------
    def checkpoint(self):
        return checkpoint_dict(self.core, self.optimizer, self.global_step)

    def save_checkpoint(self, path=None):
        if path is None:
            os.makedirs(self.logdir, exist_ok=True)
            path = os.path.join(self.logdir, '{:06d}.tar'.format(self.global_step))
        torch.save(self.checkpoint(), path)
        return path

    def load_checkpoint(self, path):
        ckpt = torch.load(path, map_location='cpu')
        self.global_step = ckpt['global_step']
        self.core.load_state_dict(ckpt['network_fn_state_dict'], strict=True)
        self.optimizer.load_state_dict(ckpt['optimizer_state_dict'])

    # ---- one iteration -----------------------------------------------------------------------------------------------------------
    def step(self, tp_input):
        """One iteration on a batch whose tensors are on the device.  Returns (loss, img_loss, acc_loss, tv_loss, l1_loss) as device
        scalars.  The tail (everything after the render backward) only enqueues work; the render before it may wait on the host as
        NeRF.render does - with n_importance > 0 it draws sample_pdf's uniforms on the CPU generator unless uniforms_on_device is set."""
        core, opt = self.core, self.optimizer
        k = 0
        rays_o, rays_d = tp_input['ray_o_all'][:, k], tp_input['ray_d_all'][:, k]
        near, far = tp_input['near_all'][:, k], tp_input['far_all'][:, k]
        target_s, bkgd_msk = tp_input['rgb_all'][:, k], tp_input['bkgd_msk_all'][:, k]
        instance_id, cloth_layer_index = tp_input['instance_idx'], tp_input['cloth_layer_index']
        planes = core.tri_planes.detach()[instance_id, cloth_layer_index].requires_grad_(True)     # the gathered copies, a leaf
        rgb, acc, _, _ = _render(chunk=self.chunk, rays_o=rays_o, rays_d=rays_d, near=near, far=far, tri_planes=planes, tp_input=tp_input,
                                 renderer=_Bare(core), n_samples=self.n_samples, perturb=self.perturb, n_importance=self.n_importance)
        img_loss = img2mse(rgb, target_s)
        acc_loss = img2mse(bkgd_msk.squeeze(2), acc)
        data_loss = img_loss + 0.1 * acc_loss
        data_loss.backward()
        if self.tail_event is not None:
            self.tail_event.record()
        grad = planes.grad
        if not grad.is_contiguous():
            grad = grad.contiguous()
        tv_loss, l1_loss = fit_reg(planes.detach(), grad, self.tv_loss_coef, self.l1_loss_coef)
        loss = data_loss.detach() + self.tv_loss_coef * tv_loss + self.l1_loss_coef * l1_loss
        if not self.ft_triplane_only:
            opt.step_mlp()
        opt.step_planes(grad, instance_id, cloth_layer_index, self.use_clamp)
        opt.zero_grad()
        if self.global_step <= LR_LAST_STEP:
            opt.param_groups[0]['lr'], opt.param_groups[1]['lr'] = lr_schedule(self.global_step, self.lrate, self.tri_plane_lrate,
                                                                               self.lrate_decay)
        self.global_step += 1
        return loss, img_loss.detach(), acc_loss.detach(), tv_loss, l1_loss

    # ---- the loop ----------------------------------------------------------------------------------------------------------------
    def run_loop(self):
        n_iters = self.n_iteration + 1
        running, count, t0, epoch = None, 0, time.time(), 0
        while self.global_step < n_iters:
            seen = 0
            for tp_input in self.data:
                seen += 1
                losses = torch.stack(self.step(tp_input)).double()
                running = losses if running is None else running + losses
                count += 1
                gs = self.global_step
                if gs % self.i_print == 0 and gs > 1:
                    r = (running / count).tolist()            # the one host read of the window
                    dt, t0, running, count = (time.time() - t0) / count, time.time(), None, 0
                    print("[TRAIN] Epoch:{}  Iter: {} Lr: {} Loss: {} Img Loss: {} Acc Loss: {} tv Loss: {} L1 Loss: {}  PSNR: {}  Time: {} s/iter"
                          .format(epoch, gs, round(self.optimizer.param_groups[0]['lr'], 6), round(r[0], 5), round(r[1], 5), round(r[2], 5),
                                  round(r[3], 5), round(r[4], 5), round(mse2psnr(r[1]), 3), round(dt, 3)), flush=True)
                if (gs % self.i_weights == 0 and gs > 1) or gs == 5000:
                    self.save_checkpoint()
                if gs >= n_iters:
                    break
            if seen == 0:
                raise RuntimeError("FitLoop: the data iterable is empty")
            epoch += 1
