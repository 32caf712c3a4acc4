"""The training loop's host side against the reference (tests/golden/train_loop_tiny32.npz from the unmodified reference TrainLoop,
gen_golden_train_loop.py), on the CPU:
  - clip + AdamW + EMA restated in float64 on the recorded gradients reproduce the reference's parameters, EMAs and moments;
  - LossSecondMomentResampler: weights, draws, warm-up and a 2-rank gloo gather;
  - _anneal_lr, checkpoint names and resume-step parsing, load_triplane_data, FusedAdamW's state_dict in torch AdamW's layout."""
import multiprocessing as mp
import os

import numpy as np
import pytest
import torch

from humanliff_amd.improved_diffusion import train_util
from humanliff_amd.improved_diffusion.resample import (LossSecondMomentResampler, UniformSampler,
                                                       create_named_schedule_sampler)
from humanliff_amd.improved_diffusion.triplane_datasets import load_triplane_data
from humanliff_amd.optim import FusedAdamW
from tests.golden_util import GOLDEN
from tests.train_loop_cases import LOOP, NSLICE, WDS

G = os.path.join(GOLDEN, "train_loop_tiny32.npz")


def _lr(step, lr=LOOP["lr"]):
    return 1e-5 + (lr - 1e-5) * (100000 - step) / 100000 if step < 100000 else None


@pytest.mark.parametrize("case", [0, 1])
def test_restated_tail_reproduces_reference(case):
    """float64 clip(0.5) -> AdamW (torch's formulas, scalars rounded to fp32 as the kernels get them) -> update_ema on the recorded
    unclipped gradients gives the reference's post-step values to fp32 rounding."""
    g = np.load(G)
    P = f"wd{case}_"
    wd = WDS[case]
    rates = [float(r) for r in LOOP["ema_rate"].split(",")]
    b1, b2, eps = 0.9, 0.999, 1e-8
    for k in map(str, g[P + "keys"]):
        p = g[P + "p0_" + k].astype(np.float64)
        m = np.zeros_like(p)
        v = np.zeros_like(p)
        e = [p.copy() for _ in rates]
        for s in range(LOOP["steps"]):
            lr = _lr(s)
            assert abs(lr - float(g[f"{P}s{s}_lr"])) < 1e-18
            gr = np.clip(g[f"{P}s{s}_g_{k}"].astype(np.float64), -0.5, 0.5)
            st = s + 1
            p = p * (1 - lr * wd)
            m = m + (1 - b1) * (gr - m)
            v = b2 * v + (1 - b2) * gr * gr
            p = p - lr / (1 - b1 ** st) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** st) + eps)
            e = [ei * r + (1 - r) * p for ei, r in zip(e, rates)]
            want = g[f"{P}s{s}_p_{k}"].astype(np.float64)
            # a few fp32 roundings per step on values of |p| ~ 0.1 and an update of ~lr
            assert np.abs(p - want).max() <= 4e-7 * max(1.0, np.abs(want).max()), (k, s, np.abs(p - want).max())
            for r, ei in zip(rates, e):
                we = g[f"{P}s{s}_e{r}_{k}"].astype(np.float64)
                assert np.abs(ei - we).max() <= 4e-7 * max(1.0, np.abs(we).max()), (k, s, r)
        wm, wv = g[f"{P}s{s}_m_{k}"], g[f"{P}s{s}_v_{k}"]
        assert np.abs(m - wm).max() <= 1e-6 * np.abs(wm).max() + 1e-12, k
        assert np.abs(v - wv).max() <= 1e-6 * np.abs(wv).max() + 1e-18, k
        assert m.size <= NSLICE


def test_grad_norm_is_unclipped_sqrt_sum():
    g = np.load(G)
    for case in (0, 1):
        assert np.all(g[f"wd{case}_grad_norm"] > 0.5)          # larger than any clipped gradient could give for these picks
    assert g["wd0_grad_norm"][0] == g["wd1_grad_norm"][0]      # step 0: weight decay cannot have acted yet


class _D:
    num_timesteps = 50


def _restated_weights(hist):
    w = np.sqrt(np.mean(hist ** 2, axis=-1))
    w = w / w.sum() * (1 - 0.001) + 0.001 / len(w)
    return w


def test_loss_second_moment_resampler_matches_reference():
    g = np.load(G)
    s = LossSecondMomentResampler(_D())
    ts, ls = g["lsm_ts"], g["lsm_losses"]
    warm = None
    for i in range(0, len(ts), 8):
        assert np.array_equal(s.weights(), np.ones(50)) or warm is not None
        s.update_with_all_losses(ts[i:i + 8].tolist(), ls[i:i + 8].tolist())
        if warm is None and s._warmed_up():
            warm = i
    assert warm is not None
    np.testing.assert_allclose(s.weights(), g["lsm_weights"], rtol=1e-15, atol=0)
    np.testing.assert_allclose(s.weights(), _restated_weights(s._loss_history), rtol=1e-12)
    np.random.seed(3)
    t, w = s.sample(16, "cpu")
    assert np.array_equal(t.numpy(), g["lsm_draw_t"])
    np.testing.assert_array_equal(w.numpy(), g["lsm_draw_w"])


def test_resampler_warmup_and_history():
    s = LossSecondMomentResampler(_D(), history_per_term=3)
    for t in range(50):
        s.update_with_all_losses([t, t], [1.0, 2.0])
    assert not s._warmed_up() and np.array_equal(s.weights(), np.ones(50))
    s.update_with_all_losses(list(range(50)), [3.0] * 50)
    assert s._warmed_up()
    s.update_with_all_losses([7], [10.0])                     # full: the oldest (1.0) drops out
    assert np.array_equal(s._loss_history[7], [2.0, 3.0, 10.0])
    assert isinstance(create_named_schedule_sampler("uniform", _D()), UniformSampler)
    assert isinstance(create_named_schedule_sampler("loss-second-moment", _D()), LossSecondMomentResampler)
    with pytest.raises(NotImplementedError):
        create_named_schedule_sampler("other", _D())


def _gather_rank(rank, path, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=2)
    s = LossSecondMomentResampler(_D())
    ts = torch.tensor([rank, 10 + rank, 20 + rank][: 2 + rank])
    s.update_with_local_losses(ts, ts.double() * 0.5)
    q.put((rank, s._loss_counts.copy(), s._loss_history[:, 0].copy()))
    dist.destroy_process_group()


def test_resampler_gathers_over_two_ranks(tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_rank, args=(r, str(tmp_path / "pg"), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = np.zeros(50, dtype=np.int64)
    want[[0, 10, 1, 11, 21]] = 1
    for _, counts, first in res:
        assert np.array_equal(counts, want)
        assert first[21] == 10.5 and first[10] == 5.0
    assert np.array_equal(res[0][2], res[1][2])


def test_anneal_lr():
    class L:
        lr = 1e-4
        resume_step = 0

        class opt:
            param_groups = [{"lr": None}]

    for step, want in ((0, 1e-4), (1, 1e-5 + (1e-4 - 1e-5) * 99999 / 100000), (99999, 1e-5 + (1e-4 - 1e-5) / 100000),
                       (100000, "same"), (150000, "same")):
        L.step = step
        L.opt.param_groups[0]["lr"] = "same"
        train_util.TrainLoop._anneal_lr(L)
        got = L.opt.param_groups[0]["lr"]
        assert got == want if isinstance(want, str) else abs(got - want) <= 1e-15 * want, (step, got)


def test_checkpoint_names_and_resume_step():
    assert train_util.checkpoint_names(20000, [0.9999, 0.99]) == ["model020000.pt", "ema_0.9999_020000.pt", "ema_0.99_020000.pt",
                                                                 "opt020000.pt"]
    assert train_util.parse_resume_step_from_filename("/a/b/model012345.pt") == 12345
    assert train_util.parse_resume_step_from_filename("/a/b/ema_0.99_000010.pt") == 0
    assert train_util.parse_resume_step_from_filename("/a/b/modelfoo.pt") == 0
    assert train_util.find_ema_checkpoint("", 3, 0.99) is None


def test_use_fp16_is_refused():
    with pytest.raises(NotImplementedError, match="use_amp"):
        train_util.TrainLoop(model=torch.nn.Linear(2, 2), diffusion=None, data=None, batch_size=1, microbatch=-1, lr=1e-4,
                             ema_rate="0.9999", log_interval=1, save_interval=1, resume_checkpoint="", use_fp16=True)


def test_load_triplane_data(tmp_path):
    L, C, H = 4, 27, 8
    planes = []
    for i in range(2):
        tp = torch.randn(1, L, 3, 9, H, H, generator=torch.Generator().manual_seed(i))
        torch.save({"network_fn_state_dict": {"tri_planes": tp}}, tmp_path / f"subj{i}.tar")
        planes.append(tp.squeeze(0).reshape(L, -1, H, H))
    (tmp_path / "human_list.txt").write_text("subj0.tar\nsubj1.tar\n")
    data = load_triplane_data(data_name="SynBody", data_dir=str(tmp_path / "x"), batch_size=8, image_size=H, num_subjects=2,
                              deterministic=True)
    x, cond, kw = next(data)
    assert x.shape == (8, C, H, H) and cond.shape == (8, C, H, H)
    for idx in range(8):
        s, layer = idx // 4, idx % 4
        assert int(kw["y"][idx]) == layer
        assert torch.equal(x[idx], planes[s][layer])
        assert torch.equal(cond[idx], planes[s][layer - 1] if layer else torch.zeros(C, H, H))
    fixed = load_triplane_data(data_name="tightcap", data_dir=str(tmp_path / "x"), batch_size=2, image_size=H, num_subjects=2,
                               layer_idx=2, deterministic=True)
    x, cond, kw = next(fixed)
    assert kw["y"].tolist() == [2, 2] and torch.equal(cond[0], planes[0][1])
    with pytest.raises(ValueError):
        next(load_triplane_data(data_name="SynBody", data_dir="", batch_size=1, image_size=H))


def test_fused_adamw_state_dict_is_adamw_layout():
    """Construction only (no step: the step needs the device): state_dicts go both ways between FusedAdamW and torch AdamW."""
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    ref = torch.optim.AdamW(ps, lr=3e-4, weight_decay=0.01)
    for p in ps:
        p.grad = torch.randn_like(p)
    ref.step()
    sd = ref.state_dict()
    f = FusedAdamW(ps, lr=1e-4, weight_decay=0.0)
    assert set(f.param_groups[0]) == set(ref.param_groups[0])
    f.load_state_dict(sd)
    assert f.param_groups[0]["lr"] == 3e-4 and f.param_groups[0]["weight_decay"] == 0.01
    for p in ps:
        assert set(f.state[p]) == {"step", "exp_avg", "exp_avg_sq"}
        assert torch.equal(f.state[p]["exp_avg_sq"], ref.state[p]["exp_avg_sq"]) and float(f.state[p]["step"]) == 1.0
    back = torch.optim.AdamW(ps, lr=1.0)
    back.load_state_dict(f.state_dict())
    assert back.state_dict()["param_groups"] == sd["param_groups"]
    assert FusedAdamW(ps).state_dict()["param_groups"][0].keys() == torch.optim.AdamW(ps).state_dict()["param_groups"][0].keys()
