"""The tri-plane FitLoop on the MI355X (humanliff_amd/recon_NeRF/fit.py, csrc/hl_fit.hip):
  - hl_fit_reg against F.l1_loss in float64 and a float64 restatement of the regularisers' gradient;
  - hl_fit_adam_planes against torch.optim.Adam on the dense index_put_(accumulate=True) gradient + clamp_, bit for bit;
  - one FitLoop.step against the PyTorch loop of INTEGRATION.md, twenty steps, the frozen decoder, resume from a checkpoint."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

from humanliff_amd import synthetic as syn
from humanliff_amd.NeRF import train as nerf_train
from humanliff_amd.recon_NeRF import Renderer, render
from humanliff_amd.recon_NeRF.fit import FitAdam, FitLoop, fit_reg, split_parameters

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TV, L1 = 1e-2, 5e-4


def same_bits(a, b):
    return torch.equal(a, b) or (torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num()))


# ---- hl_fit_reg -----------------------------------------------------------------------------------------------------------------
def sign64(d):
    """sign with 0 at 0 and NaN kept (torch.sign maps NaN to 0)."""
    return torch.where(d.isnan(), d, d.sign())


def reg_restatement(x, g0, tv, l1):
    """float64: the three means of run_nerf_batch.py:256-259, the gradient g0 + tv d(tv_x + tv_y) + l1 d(l1), and per element the sum of
    the absolute values of the terms that make it up."""
    xd = x.double()
    dh, dw = xd[..., :-1, :] - xd[..., 1:, :], xd[..., :, :-1] - xd[..., :, 1:]
    sh, sw, s0 = sign64(dh) * (tv / dh.numel()), sign64(dw) * (tv / dw.numel()), sign64(xd) * (l1 / xd.numel())
    g, a = g0.double().clone(), g0.double().abs()
    g[..., :-1, :] += sh
    g[..., 1:, :] -= sh
    g[..., :, :-1] += sw
    g[..., :, 1:] -= sw
    g += s0
    a[..., :-1, :] += sh.abs()
    a[..., 1:, :] += sh.abs()
    a[..., :, :-1] += sw.abs()
    a[..., :, 1:] += sw.abs()
    a += s0.abs()
    tv_loss = F.l1_loss(xd[..., 0:-1, :], xd[..., 1:, :]) + F.l1_loss(xd[..., :, 0:-1], xd[..., :, 1:])
    l1_loss = F.l1_loss(xd, torch.zeros_like(xd))
    return tv_loss, l1_loss, g, a


def reg_case(bs, hw, seed, nan):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((bs, 3, 9, hw, hw), generator=g) * 0.6).clamp_(-1, 1)      # (a good share of the values sits at -1 and 1)
    x[0, 0, 0, 0, :4] = 0.0                                  # exact zeros, equal to their neighbours along W
    x[-1, 2, 8, -1, -1] = 0.0
    x[0, 1, 3, 2:5, 3] = 0.25                                # equal neighbours along H
    x[0, 2, 4, 1, 1], x[0, 2, 4, 1, 2] = 1.0, -1.0
    x[0, 0, 1, 3, 3] = -0.0
    if nan:
        x[-1, 1, 5, hw // 2, hw // 2] = float("nan")
        x[0, 0, 0, 0, 0] = float("nan")                      # a corner: two neighbours only
    g0 = torch.randn(x.shape, generator=g) * 1e-4
    g0[0, 0, 0, 1, :] = 0.0
    return x.to(DEV), g0.to(DEV)


@pytest.mark.parametrize("bs", [1, 2, 8])
@pytest.mark.parametrize("hw", [8, 64, 256])
def test_fit_reg_matches_float64(hw, bs):
    for nan in (False, True):
        x, g0 = reg_case(bs, hw, 100 * hw + bs, nan)
        grad = g0.clone()
        tv_loss, l1_loss = fit_reg(x, grad, TV, L1)
        want_tv, want_l1, want_g, terms = reg_restatement(x, g0, TV, L1)
        assert tv_loss.dtype == torch.float32 and l1_loss.dtype == torch.float32 and tv_loss.is_cuda
        for name, got, want in (("tv", tv_loss, want_tv), ("l1", l1_loss, want_l1)):
            got, want = float(got), float(want)
            print(f"hw {hw} bs {bs} nan {nan}: {name}_loss {got!r} float64 {want!r} relative {abs(got - want) / want if want == want else float('nan'):.3e}")
            if nan:
                assert got != got and want != want            # a NaN texel makes both means NaN
            else:
                assert abs(got - want) <= 2.0 ** -23 * abs(want), (name, got, want)
        assert torch.equal(torch.isnan(grad), torch.isnan(want_g)), "NaN must sit where the float64 gradient has it"
        assert bool(torch.isnan(grad).any()) == nan
        ok = ~torch.isnan(want_g)
        err, bound = (grad.double() - want_g).abs()[ok], (8 * 2.0 ** -24 * terms)[ok]
        print(f"hw {hw} bs {bs} nan {nan}: worst gradient error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all())
        # sign(0) = 0: an all-zero image with a zero gradient stays zero, whatever its neighbours in memory hold
        if not nan:
            z, gz = torch.zeros_like(x), torch.zeros_like(x)
            tvz, l1z = fit_reg(z, gz, TV, L1)
            assert float(tvz) == 0.0 and float(l1z) == 0.0 and not bool(gz.any())
        again = g0.clone()
        tv2, l12 = fit_reg(x, again, TV, L1)
        assert same_bits(again, grad) and same_bits(tv2, tv_loss) and same_bits(l12, l1_loss)


def test_fit_reg_unaligned_width_and_bad_arguments():
    """W % 4 != 0 takes the element-wise path; CPU tensors and mismatched shapes raise."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 3, 9, 7, 10), generator=g).to(DEV)
    g0 = (torch.randn(x.shape, generator=g) * 1e-4).to(DEV)
    grad = g0.clone()
    tv_loss, l1_loss = fit_reg(x, grad, TV, L1)
    want_tv, want_l1, want_g, terms = reg_restatement(x, g0, TV, L1)
    assert abs(float(tv_loss) - float(want_tv)) <= 2.0 ** -23 * float(want_tv)
    assert abs(float(l1_loss) - float(want_l1)) <= 2.0 ** -23 * float(want_l1)
    assert bool(((grad.double() - want_g).abs() <= 8 * 2.0 ** -24 * terms).all())
    with pytest.raises(RuntimeError):
        fit_reg(x.cpu(), grad.cpu(), TV, L1)
    with pytest.raises(RuntimeError):
        fit_reg(x, grad[:1], TV, L1)


# ---- hl_fit_adam_planes ---------------------------------------------------------------------------------------------------------
INDEX_SETS = [([0, 2], [1, 3]), ([1, 1, 1], [2, 2, 2]), ([0, 2, 0, 2], [1, 3, 0, 3]), ([2], [0]), ([-1, 0], [-1, 1])]
LRS = [1e-2 * (1 - 0.1 * s) for s in range(5)]


def planes_case(ni, dim, seed):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn((ni, 4, 3, 9, dim, dim), generator=g) * 0.7
    steps = []
    for s, (inst, layer) in enumerate(INDEX_SETS):
        inst = [min(i, ni - 1) if i >= 0 else i for i in inst]           # (one instance: every entry selects it, more duplicates)
        bufs = torch.randn((len(inst), 3, 9, dim, dim), generator=g) * (0.5 + s)
        if s == 2:
            bufs[0, 0, 0, 0, 0], bufs[1, 1, 1, 1, 1], bufs[2, 2, 2, 2, 2] = float("inf"), float("nan"), -float("inf")
        steps.append((torch.tensor(inst), torch.tensor(layer), bufs))
    return p0, steps


def run_planes_fused(p0, steps, clamp):
    p = torch.nn.Parameter(p0.clone().to(DEV))
    opt = FitAdam([], p, 5e-4, 1e-2)
    out = []
    for s, (inst, layer, bufs) in enumerate(steps):
        opt.param_groups[1]['lr'] = LRS[s]
        opt.step_planes(bufs.to(DEV), inst.to(DEV), layer.to(DEV), clamp)
        out.append((p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()))
    return out, p, opt


def run_planes_torch(p0, steps, clamp, foreach):
    p = torch.nn.Parameter(p0.clone().to(DEV))
    opt = torch.optim.Adam([p], lr=1e-2, betas=(0.9, 0.999), foreach=foreach)
    out = []
    for s, (inst, layer, bufs) in enumerate(steps):
        dense = torch.zeros_like(p)
        bufs = bufs.to(DEV)
        for b in range(len(inst)):                            # index_put_(accumulate=True) with the order fixed: batch order
            dense[int(inst[b]), int(layer[b])] += bufs[b]
        p.grad = dense
        opt.param_groups[0]['lr'] = LRS[s]
        opt.step()
        if clamp:
            p.data.clamp_(-1.0, 1.0)
        out.append((p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()))
    return out


def rel(a, b):
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b))
    f = torch.isfinite(b)
    return float((a[f].double() - b[f].double()).abs().max() / b[f].double().abs().max().clamp_min(1e-30)) if f.any() else 0.0


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("ni,dim", [(1, 32), (3, 32), (3, 5)])        # 27 * 32 * 32 elements: one whole chunk and a part; 5 x 5: no float4 path
def test_fit_adam_planes_matches_torch_adam(ni, dim, clamp):
    p0, steps = planes_case(ni, dim, seed=7 + ni)
    got, _, _ = run_planes_fused(p0, steps, clamp)
    for foreach in (True, False):
        want = run_planes_torch(p0, steps, clamp, foreach)
        for s in range(5):
            for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got[s], want[s]):
                # bit-identical to the multi-tensor path whose op order the kernel follows; the single-tensor path rounds differently
                # (no fma) and is held to the relative bound test_fused_step_matches_torch_adamw holds it to
                if foreach:
                    assert same_bits(a, b), f"step {s + 1}: {name} differs from torch.optim.Adam(foreach=True)"
                assert rel(a, b) <= 1e-6, f"step {s + 1} (foreach={foreach}): {name}"
    if clamp:
        f = torch.isfinite(got[-1][0])
        assert float(got[-1][0][f].abs().max()) <= 1.0


def test_fit_adam_planes_index_put_reference_and_no_host_sync():
    """The batch-order sum is what index_put_(accumulate=True) builds when no slice repeats; the step reads no index on the host."""
    p0, steps = planes_case(3, 32, seed=11)
    inst, layer, bufs = steps[0]
    p = torch.nn.Parameter(p0.clone().to(DEV))
    ref = torch.optim.Adam([p], lr=LRS[0], betas=(0.9, 0.999), foreach=True)
    p.grad = torch.zeros_like(p).index_put_((inst.to(DEV), layer.to(DEV)), bufs.to(DEV), accumulate=True)
    ref.step()
    got, q, opt = run_planes_fused(p0, steps[:1], False)
    assert same_bits(got[0][0], p.detach()) and same_bits(got[0][1], ref.state[p]["exp_avg"])
    a, _, _ = run_planes_fused(p0, steps, True)
    b, q, opt = run_planes_fused(p0, steps, True)
    for x, y in zip(a, b):
        assert all(same_bits(u, v) for u, v in zip(x, y))
    inst, layer, bufs = (t.to(DEV) for t in steps[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            opt.step_planes(bufs, inst, layer, True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        opt.step_planes(bufs, inst.cpu(), layer, True)
    with pytest.raises(RuntimeError):
        opt.step_planes(bufs, inst.int(), layer.int(), True)


# ---- the whole step -------------------------------------------------------------------------------------------------------------
KW = dict(lrate=5e-4, tri_plane_lrate=1e-2, lrate_decay=10, tv_loss_coef=TV, l1_loss_coef=L1, use_clamp=True, n_samples=16,
          n_importance=16, perturb=1., chunk=1024 * 32, i_print=5, i_weights=1000)


def small_model(seed=0):
    torch.manual_seed(seed)
    r = Renderer(use_canonical_space=False, num_instances=3, triplane_dim=64, triplane_ch=27, test=False)
    r.load_state_dict(syn.render_mlp_state(3), strict=False)
    return r.to(DEV)


def batch(seed=41, bs=2, **kw):
    return {k: v.to(DEV) for k, v in syn.fit_batch(bs, 256, 3, seed=seed, **kw).items()}


def state_of(loop):
    """Every parameter and every optimizer-state tensor, in a fixed order."""
    out = [p.detach().clone() for p in loop.core.parameters()]
    for grp in loop.optimizer.param_groups:
        for p in grp['params']:
            st = loop.optimizer.state.get(p, {})
            out += [st[k].detach().clone().to(DEV) for k in ("step", "exp_avg", "exp_avg_sq") if k in st]
    return out


def torch_loop_step(model, opt, tp, kw):
    """run_nerf_batch.py:236-272 as INTEGRATION.md prescribed it before FitLoop: HIP render forward / backward, torch TV / L1, Adam, clamp_."""
    k = 0
    rgb, acc, _, _ = render(chunk=kw["chunk"], rays_o=tp['ray_o_all'][:, k], rays_d=tp['ray_d_all'][:, k], tp_input=tp, near=tp['near_all'][:, k],
                            far=tp['far_all'][:, k], renderer=model, n_samples=kw["n_samples"], perturb=kw["perturb"], n_importance=kw["n_importance"])
    ii, ll = tp['instance_idx'], tp['cloth_layer_index']
    img_loss = torch.mean((rgb - tp['rgb_all'][:, k]) ** 2)
    acc_loss = torch.mean((tp['bkgd_msk_all'][:, k].squeeze(2) - acc) ** 2)
    tri = model.tri_planes
    tv_loss = F.l1_loss(tri[ii, ll, :, :, 0:-1, :], tri[ii, ll, :, :, 1:, :]) + F.l1_loss(tri[ii, ll, :, :, :, 0:-1], tri[ii, ll, :, :, :, 1:])
    l1_loss = F.l1_loss(tri[ii, ll], torch.zeros_like(tri[ii, ll]))
    loss = img_loss + 0.1 * acc_loss + kw["tv_loss_coef"] * tv_loss + kw["l1_loss_coef"] * l1_loss
    loss.backward()
    grads = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
    opt.step()
    opt.zero_grad()
    if kw["use_clamp"]:
        tri.data.clamp_(-1.0, 1.0)
    return [t.detach() for t in (loss, img_loss, acc_loss, tv_loss, l1_loss)], grads


def create_adam(model, kw, foreach=True):
    mlp, tri = split_parameters(model)
    return torch.optim.Adam([{'params': mlp, 'lr': kw["lrate"]}, {'params': [tri], 'lr': kw["tri_plane_lrate"]}], betas=(0.9, 0.999), foreach=foreach)


def test_one_step_against_the_pytorch_loop():
    base = small_model()
    tp = batch(instance_idx=[0, 2], layer_idx=[1, 3])
    # the PyTorch loop on a deep copy
    ref = copy.deepcopy(base)
    ref_opt = create_adam(ref, KW)
    torch.manual_seed(5)
    want_losses, ref_grads = torch_loop_step(ref, ref_opt, tp, KW)
    # FitLoop, with the gradients it hands to its two launches recorded
    model = copy.deepcopy(base)
    loop = FitLoop(model, [tp], **KW)
    seen = {}
    step_mlp, step_planes = loop.optimizer.step_mlp, loop.optimizer.step_planes
    mlp, tri = split_parameters(model)

    def rec_mlp():
        seen["mlp"] = [p.grad.clone() for p in mlp]
        step_mlp()

    def rec_planes(grad, inst, layer, clamp):
        seen["planes"] = grad.clone()
        step_planes(grad, inst, layer, clamp)

    loop.optimizer.step_mlp, loop.optimizer.step_planes = rec_mlp, rec_planes
    torch.manual_seed(5)
    got_losses = loop.step(tp)
    assert loop.global_step == 1 and all(p.grad is None for p in model.parameters())
    # the five losses: within 2^-23 relative, test_fit_reg_matches_float64's bound
    for name, g, w in zip(("loss", "img", "acc", "tv", "l1"), got_losses, want_losses):
        g, w = float(g), float(w)
        print(f"{name}_loss FitLoop {g!r} PyTorch loop {w!r} relative {abs(g - w) / abs(w):.3e}")
    for name, g, w in zip(("loss", "img", "acc", "tv", "l1"), got_losses, want_losses):
        assert abs(float(g) - float(w)) <= 2.0 ** -23 * abs(float(w)), name
    # the assembled per-slice gradient: the bound of test_fit_reg_matches_float64 plus one ulp of the render gradient
    ii, ll = tp['instance_idx'], tp['cloth_layer_index']
    dense = torch.zeros_like(tri)
    for b in range(len(ii)):
        dense[int(ii[b]), int(ll[b])] += seen["planes"][b]
    want_dense = ref_grads[[n for n, _ in ref.named_parameters()].index('tri_planes')]
    x = base.tri_planes.detach()[ii, ll]
    _, _, reg_only, reg_terms = reg_restatement(x, torch.zeros_like(x), TV, L1)
    render_part = (want_dense[ii, ll].double() - reg_only).abs()
    bound = 8 * 2.0 ** -24 * (render_part + reg_terms) + 2.0 ** -23 * render_part
    err = (seen["planes"].double() - want_dense[ii, ll].double()).abs()
    print(f"per-slice gradient: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    untouched = torch.ones(tri.shape[:2], dtype=torch.bool)
    untouched[ii.cpu(), ll.cpu()] = False
    assert not bool(want_dense[untouched].any()) and not bool(dense[untouched].any())
    for g, w in zip(seen["mlp"], [gr for (n, _), gr in zip(ref.named_parameters(), ref_grads) if n != 'tri_planes']):
        assert torch.equal(g, w)                              # the same HIP backward: the same bits
    # given FitLoop's own gradient, torch's Adam + clamp_ lands on the same bits
    twin = copy.deepcopy(base)
    twin_opt = create_adam(twin, KW)
    tmlp, ttri = split_parameters(twin)
    for p, g in zip(tmlp, seen["mlp"]):
        p.grad = g
    ttri.grad = dense
    twin_opt.step()
    ttri.data.clamp_(-1.0, 1.0)
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.equal(p.detach(), q.detach())
    for p, q in zip(mlp + [tri], tmlp + [ttri]):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(loop.optimizer.state[p][k], twin_opt.state[q][k])
        assert float(loop.optimizer.state[p]["step"]) == float(twin_opt.state[q]["step"]) == 1.0


def run_steps(base, n, seed, **over):
    model = copy.deepcopy(base)
    tps = [batch(41), batch(43, instance_idx=[1, 1], layer_idx=[2, 2])]
    loop = FitLoop(model, tps, **{**KW, **over})
    torch.manual_seed(seed)
    losses = [loop.step(tps[i % 2]) for i in range(n)]
    return loop, torch.stack([torch.stack(l) for l in losses]).cpu()


def test_twenty_steps_decrease_reproduce_and_freeze():
    base = small_model()
    before = nerf_train.LAUNCHES["hl_render_weight_grads"]
    loop, losses = run_steps(base, 20, seed=9)
    assert nerf_train.LAUNCHES["hl_render_weight_grads"] == before + 20 * 2      # one per subject and step
    total = losses[:, 0]
    print("total loss per step:", [round(float(v), 6) for v in total])
    assert bool(torch.isfinite(losses).all()) and float(total[-4:].mean()) < float(total[:4].mean())
    assert float(loop.core.tri_planes.detach().abs().max()) <= 1.0
    loop2, losses2 = run_steps(base, 20, seed=9)
    assert torch.equal(losses, losses2)
    for a, b in zip(state_of(loop), state_of(loop2)):
        assert torch.equal(a, b)
    # frozen decoder: no MLP tensor moves, no weight-gradient launch, the planes still fit
    before = nerf_train.LAUNCHES["hl_render_weight_grads"]
    ft, ft_losses = run_steps(base, 20, seed=9, ft_triplane_only=True, lrate=0.0)
    assert nerf_train.LAUNCHES["hl_render_weight_grads"] == before
    for (n, p), (_, q) in zip(ft.core.named_parameters(), base.named_parameters()):
        assert torch.equal(p.detach(), q.detach()) == (n != 'tri_planes'), n
        assert p.requires_grad == (n == 'tri_planes')
    assert len(ft.optimizer.state_dict()['state']) == 1
    assert float(ft_losses[-4:, 0].mean()) < float(ft_losses[:4, 0].mean())


def test_resume_is_bit_identical(tmp_path):
    base = small_model()
    tps = [batch(41), batch(43, instance_idx=[1, 1], layer_idx=[2, 2]), batch(47)]
    kw = {**KW, "basedir": str(tmp_path), "expname": "run", "i_weights": 6}

    def six(loop):
        for i in range(6):
            loop.step(tps[(loop.global_step) % 3])

    loop = FitLoop(copy.deepcopy(base), tps, **kw)
    torch.manual_seed(3)
    six(loop)
    path = loop.save_checkpoint()
    assert os.path.basename(path) == "000006.tar"
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(DEV))
    six(loop)
    # a fresh loop finds the run's newest checkpoint, like create_nerf
    again = FitLoop(copy.deepcopy(base), tps, **kw)
    assert again.global_step == 6
    assert again.optimizer.param_groups[1]['lr'] == loop_lr(5, kw)
    torch.set_rng_state(rng[0])
    torch.cuda.set_rng_state(rng[1], DEV)
    six(again)
    assert again.global_step == loop.global_step == 12
    for a, b in zip(state_of(loop), state_of(again)):
        assert torch.equal(a, b)
    # the same file loads into the reference script's optimizer
    ck = torch.load(path, map_location='cpu')
    assert list(ck) == ['global_step', 'network_fn_state_dict', 'optimizer_state_dict']
    ref = copy.deepcopy(base)
    ref.load_state_dict(ck['network_fn_state_dict'], strict=True)
    adam = create_adam(ref, KW)
    adam.load_state_dict(ck['optimizer_state_dict'])
    assert float(adam.state[ref.tri_planes]["step"]) == 6.0
    assert adam.state[ref.tri_planes]["exp_avg"].device == ref.tri_planes.device


def loop_lr(step, kw):
    return kw["tri_plane_lrate"] * (0.5 ** (step / (kw["lrate_decay"] * 60)))
