"""The HIP training path of the 3-D-aware and cross-attention UNets (csrc/hl_unet_train_xf.hip, improved_diffusion/unet_train.py):
the new kernels against float64 autograd on the CPU, GaussianDiffusion.training_losses(...).backward() against the REFERENCE's loss
and gradients (tests/golden/train_loss_variants.npz <- tests/golden/gen_golden_train_variants.py), every parameter gradient against the
PyTorch-op twin on the GPU, and the optimizer / graph / autocast / guidance modes."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from tests.test_train_variants_cpu import build
from tests.train_variants_cases import CASES, case_inputs
from tests.unet_autograd_twin import forward_autograd

from tests.golden_util import GOLDEN
from humanliff_amd.improved_diffusion import unet_train as ut

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


def rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max())


# ---- kernel units: float64 autograd on the CPU is the reference ---------------------------------------------------------------------
def agg64(g):
    """unet.py:208-214 on NHWC (N, H, 3W, C): the planes side by side, silu(cat[own, two plane means])."""
    w = g.shape[2] // 3
    p0, p1, p2 = g[:, :, :w], g[:, :, w:2 * w], g[:, :, 2 * w:]
    row = lambda p: p.mean(2, keepdim=True).expand(-1, -1, w, -1)                 # noqa: E731   mean over the columns, per row
    col = lambda p: p.mean(1, keepdim=True).expand(-1, p.shape[1], -1, -1)        # noqa: E731   mean over the rows, per column
    out = torch.cat([torch.cat([p0, row(p1), col(p2)], -1), torch.cat([p1, row(p0), row(p2)], -1), torch.cat([p2, col(p0), col(p1)], -1)], 2)
    return F.silu(out)


def check_unit(fn, ref, inputs, fwd_tol, bwd_tol):
    """fn on the GPU vs ref in float64 on the CPU: output and every input gradient for a random output gradient; fn twice gives the same bits."""
    gen = torch.Generator().manual_seed(3)
    xs = [t.double().requires_grad_(True) for t in inputs]
    want = ref(*xs)
    dout = torch.randn(want.shape, generator=gen, dtype=torch.float64)
    want_g = torch.autograd.grad(want, xs, dout)
    runs = []
    for _ in range(2):
        xg = [t.float().to(dev).requires_grad_(True) for t in inputs]
        got = fn(*xg)
        runs.append((got.detach(), torch.autograd.grad(got, xg, dout.float().to(dev))))
    got, got_g = runs[0]
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1])), "not bit-reproducible"
    assert rel(got, want) < fwd_tol, rel(got, want)
    for i, (a, b) in enumerate(zip(got_g, want_g)):
        assert rel(a, b) < bwd_tol, (i, rel(a, b))


@pytest.mark.parametrize("N,H,C", [(2, 32, 32), (2, 16, 64), (2, 8, 128), (1, 64, 192), (1, 5, 12)])
def test_triplane_aggregation_matches_float64(N, H, C):
    g = torch.randn((N, H, 3 * H, C), generator=torch.Generator().manual_seed(N * H + C)) * 2
    check_unit(lambda t: ut._TriplaneAgg.apply(t), agg64, [g], 2e-6, 2e-5)


def test_triplane_aggregation_refuses_rectangular_planes():
    with pytest.raises(Exception, match="hl_triplane_agg_forward"):
        ut._TriplaneAgg.apply(torch.zeros((1, 4, 15, 8), device=dev))


@pytest.mark.parametrize("P,C", [(2048, 64), (512, 128), (128, 256), (37, 20)])
def test_layernorm_matches_float64(P, C):
    gen = torch.Generator().manual_seed(P + C)
    x = torch.randn((P, C), generator=gen) * 3 + 0.5
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen)
    check_unit(lambda a, gm, bt: ut._LayerNorm.apply(a.reshape(1, 1, P, C), gm, bt, 1e-5).reshape(P, C),
               lambda a, gm, bt: F.layer_norm(a, (C,), gm, bt, 1e-5), [x, gamma, beta], 5e-6, 2e-5)


@pytest.mark.parametrize("P,F_", [(2048, 256), (1024, 512), (33, 7)])
def test_geglu_matches_float64(P, F_):
    p = torch.randn((P, 2 * F_), generator=torch.Generator().manual_seed(P)) * 2
    ref = lambda t: t[:, :F_] * F.gelu(t[:, F_:])  # noqa: E731
    check_unit(lambda t: ut._GEGLU.apply(t), ref, [p], 2e-6, 5e-6)


@pytest.mark.parametrize("N,H,W,C", [(2, 32, 32, 64), (2, 8, 8, 128), (1, 5, 7, 96)])
def test_groupnorm_with_eps_matches_float64(N, H, W, C):
    """SpatialTransformer.norm: GroupNorm(32, eps 1e-6).  Inputs of variance ~1e-6, where the eps decides the result."""
    gen = torch.Generator().manual_seed(N * H + C)
    x = torch.randn((N, H, W, C), generator=gen) * 1e-3
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen)
    ref = lambda a, gm, bt: F.group_norm(a.permute(0, 3, 1, 2), 32, gm, bt, 1e-6).permute(0, 2, 3, 1)  # noqa: E731
    check_unit(lambda a, gm, bt: ut._GroupNormAct.apply(a, gm, bt, None, False, 1e-6), ref, [x, gamma, beta], 1e-5, 2e-4)
    with torch.no_grad():                     # the eps is the one asked for: GroupNorm32's 1e-5 gives another result on these inputs
        y5 = ut._GroupNormAct.apply(x.to(dev), gamma.to(dev), beta.to(dev), None, False, None)
        y6 = ut._GroupNormAct.apply(x.to(dev), gamma.to(dev), beta.to(dev), None, False, 1e-6)
    assert float((y5 - y6).abs().max()) > 0.1 * float(y6.abs().max())


# ---- the networks --------------------------------------------------------------------------------------------------------------------
def hip_case(tag):
    model, diffusion = build(tag)
    x0, xc, t, y, noise = case_inputs(tag)
    to = lambda v: None if v is None else v.to(dev)  # noqa: E731
    return model.to(dev).train(), diffusion, (to(x0), to(xc), to(t), to(y), to(noise))


def train_loss(model, diffusion, batch, fn=None):
    x0, xc, t, y, noise = batch
    m = model if fn is None else (lambda x, ts, x_cond=None, y=None: fn(model, x, ts, x_cond, y))
    return diffusion.training_losses(m, x0, xc, t, model_kwargs={"y": y}, noise=noise)["loss"]


@pytest.mark.parametrize("tag", CASES)
def test_training_losses_backward_matches_reference_on_hip(tag):
    """training_losses -> backward() through UNetModel.forward on the GPU (the HIP training path; the twin lives under tests/ and the
    product cannot reach it) against the reference's loss and gradients.  Bounds of test_unet_train_gpu.py's controlnet test: loss 1e-5,
    2e-4 of each tensor's largest entry; the zero gradients of attn2.to_q / to_k / norm2 are exact zero tensors."""
    g = np.load(os.path.join(GOLDEN, "train_loss_variants.npz"))
    model, diffusion, batch = hip_case(tag)
    loss = train_loss(model, diffusion, batch)
    assert loss.requires_grad
    lerr = float(np.abs(loss.detach().cpu().numpy() - g[f"{tag}_loss"]).max())
    assert lerr < 1e-5, lerr
    loss.mean().backward()
    sd = dict(model.named_parameters())
    assert all(p.grad is not None for p in sd.values())
    tot = sum(float(p.grad.double().abs().sum()) for p in sd.values())
    ref_tot = float(g[f"{tag}_grad_abs_sum"])
    assert abs(tot - ref_tot) < 2e-4 * ref_tot, (tot, ref_tot)
    worst, zeros = 0.0, 0
    for k in map(str, g[f"{tag}_keys"]):
        ref = torch.from_numpy(g[f"{tag}_g_{k}"])
        if not ref.abs().max() > 0:
            assert torch.equal(sd[k].grad.cpu(), torch.zeros_like(ref)), k
            zeros += 1
            continue
        err = rel(sd[k].grad, ref)
        worst = max(worst, err)
        assert err < 2e-4, (k, err)
    assert zeros == (4 if tag == "xattn" else 0)
    print(f"{tag} on HIP vs reference: loss max-abs {lerr:.2e}, worst relative gradient error {worst:.2e}, "
          f"sum|grad| rel {abs(tot - ref_tot) / ref_tot:.2e}")


@pytest.mark.parametrize("tag", CASES)
def test_every_gradient_matches_twin_and_is_bit_reproducible(tag):
    """Every parameter gradient against the PyTorch-op twin on the GPU (MIOpen / rocBLAS), with the bound and the floor of
    test_unet_train_gpu.py::test_training_other_cond_types_on_hip; two HIP backward passes give identical gradients."""
    model, diffusion, batch = hip_case(tag)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        loss = train_loss(model, diffusion, batch)
        loss.mean().backward()
        runs.append({k: p.grad.clone() for k, p in model.named_parameters()})
    diff = [k for k in runs[0] if not torch.equal(runs[0][k], runs[1][k])]
    assert not diff, diff
    model.zero_grad(set_to_none=True)
    loss_t = train_loss(model, diffusion, batch, forward_autograd)
    loss_t.mean().backward()
    assert float((loss.detach() - loss_t.detach()).abs().max()) < 1e-5 * max(1.0, float(loss_t.detach().abs().max()))
    gscale = max(float(p.grad.abs().max()) for p in model.parameters())
    worst = 0.0
    for k, p in model.named_parameters():
        scale = max(float(p.grad.abs().max()), 1e-4 * gscale)
        err = float((runs[0][k] - p.grad).abs().max()) / scale
        worst = max(worst, err)
        assert err < 3e-3, (k, err)
    print(f"{tag}: HIP training path vs twin, worst relative gradient error {worst:.2e}")


@pytest.mark.parametrize("tag", ["aware3d_controlnet", "xattn"])
def test_adamw_steps_lower_loss_and_sampling_sees_them(tag):
    model, diffusion, batch = hip_case(tag)
    x0, xc, t, y, _ = batch
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, fused=True)
    with torch.no_grad():
        model.eval()
        before = model(x0, t, xc, y=y)
        model.train()
    losses = []
    for _ in range(4):
        opt.zero_grad(set_to_none=True)
        loss = train_loss(model, diffusion, batch).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses
    model.eval()
    with torch.no_grad():
        after = model(x0, t, xc, y=y)
        twin = forward_autograd(model, x0, t, xc, y=y)
    assert (after - before).abs().max() > 1e-3
    assert (after - twin).abs().max() < 1e-4 * max(1.0, float(twin.abs().max()))


@pytest.mark.parametrize("tag", ["aware3d_concat", "xattn"])
def test_graphed_train_step_equals_eager_steps(tag):
    from humanliff_amd.improved_diffusion.unet_train import GraphedTrainStep
    x0, xc, _, y, _ = hip_case(tag)[2]
    gen = torch.Generator().manual_seed(11)
    batches = [((x0 + 0.1 * torch.randn(x0.shape, generator=gen).to(dev)).clamp(-1, 1), torch.randint(0, 1000, (2,), generator=gen).to(dev),
                torch.randn(x0.shape, generator=gen).to(dev)) for _ in range(3)]

    def fresh():
        model, diffusion, _ = hip_case(tag)
        return model, diffusion, torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01, fused=True, capturable=True)

    m1, d1, o1 = fresh()
    eager = []
    for x, t, n in batches:
        o1.zero_grad(set_to_none=True)
        loss = d1.training_losses(m1, x, xc, t, model_kwargs={"y": y}, noise=n)["loss"].mean()
        loss.backward()
        o1.step()
        eager.append(float(loss.detach()))
    del loss
    m2, d2, o2 = fresh()
    step = GraphedTrainStep(d2, m2, o2, batches[0][0], xc, batches[0][1], {"y": y}, with_noise=True)
    graphed = [float(step(x, xc, t, {"y": y}, noise=n)) for x, t, n in batches]
    assert graphed == eager, (graphed, eager)
    bad = [k for (k, a), b in zip(m1.named_parameters(), m2.parameters()) if not torch.equal(a, b)]
    assert not bad, bad


@pytest.mark.parametrize("tag", ["aware3d_controlnet", "xattn"])
def test_training_under_autocast_tracks_fp32(tag):
    """Under torch.autocast(bfloat16) the convolutions take bf16 operands where they already do; the new kernels stay fp32.  Bounds of
    test_unet_train_gpu.py::test_training_under_autocast_and_in_bf16_arithmetic_tracks_fp32."""
    model, diffusion, batch = hip_case(tag)
    grads, losses = [], []
    for amp in (False, True):
        model.zero_grad(set_to_none=True)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=amp):
            loss = train_loss(model, diffusion, batch).mean()
        assert loss.dtype == torch.float32
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append({k: p.grad.clone() for k, p in model.named_parameters()})
    assert abs(losses[1] - losses[0]) < 2e-3 * abs(losses[0]), losses
    num = sum(float(((grads[1][k] - grads[0][k]).double() ** 2).sum()) for k in grads[0])
    den = sum(float((grads[0][k].double() ** 2).sum()) for k in grads[0])
    assert (num / den) ** 0.5 < 3e-2, (num / den) ** 0.5


@pytest.mark.parametrize("tag", ["aware3d_plain", "xattn"])
def test_eval_mode_input_gradient(tag):
    model, _, (x0, xc, t, y, _) = hip_case(tag)
    model.eval()
    x = x0.clone().requires_grad_(True)
    out = model(x, t, xc, y=y)
    assert out.requires_grad
    (gx,) = torch.autograd.grad(out.square().sum(), x)
    xt = x0.clone().requires_grad_(True)
    (gt,) = torch.autograd.grad(forward_autograd(model, xt, t, xc, y=y).square().sum(), xt)
    assert (gx - gt).abs().max() < 5e-4 * float(gt.abs().max())
