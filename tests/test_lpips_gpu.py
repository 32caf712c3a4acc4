"""hl_lpips on the MI355X (humanliff_amd/lpips.py, csrc/hl_lpips.hip) against the float64 restatement of LPIPS(net='vgg')
(tests/lpips_restatement.py) on seeded random weights, and evaluate_views with an LpipsVGG as its lpips_fn.

Bounds (tests/lpips_cases.py): the tap features, each d_k and the total may differ from float64 by 3.5 x what the restatement run in
float32 on the CPU differs from it, pooled over the cases."""
import json

import numpy as np
import pytest
import torch

from humanliff_amd import synthetic as syn
from humanliff_amd.lpips import LpipsVGG
from tests import lpips_cases as lc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def model():
    convs, lins = lc.weights()
    return LpipsVGG(convs, lins, device=DEV)


@pytest.mark.parametrize("name", list(lc.CASES))
def test_case_matches_the_restatement(model, name):
    in0, in1 = (t.to(DEV) for t in lc.case(name))
    keep0, keep1 = in0.clone(), in1.clone()
    want = lc.reference(name)
    f0, f1 = model.features(in0), model.features(in1)
    val, terms = model(in0, in1, retPerLayer=True)
    assert val.shape == (1, 1, 1, 1) and val.dtype == torch.float32 and val.is_cuda and len(terms) == 5
    for k in range(5):
        assert f0[k].shape == want["f0"][k].shape and terms[k].shape == (1, 1, 1, 1), k
    feat, term, total = lc.errors([f.cpu() for f in f0], [f.cpu() for f in f1], [t.cpu() for t in terms], val.cpu(), want)
    print(f"{name}: total {float(val)!r} (float64 {want['total']!r}) relative error {total:.3e} (bound {lc.TOTAL_BOUND:.1e}); largest term "
          f"error {term:.3e} (bound {lc.TERM_BOUND:.1e}); feature errors over abs-max {['%.3e' % f for f in feat]} "
          f"(bounds {['%.1e' % b for b in lc.FEATURE_BOUND]})")
    for k in range(5):
        assert feat[k] <= lc.FEATURE_BOUND[k], (name, k)
    assert term <= lc.TERM_BOUND, name
    assert total <= lc.TOTAL_BOUND, name
    assert torch.equal(in0, keep0) and torch.equal(in1, keep1), "the inputs are only read"


def test_identity_and_symmetry(model):
    in0, in1 = (t.to(DEV) for t in lc.case("37x50"))
    val, terms = model(in0, in0.clone(), retPerLayer=True)
    assert float(val) == 0.0 and all(float(t) == 0.0 for t in terms)
    ab, ab_terms = model(in0, in1, retPerLayer=True)
    ba, ba_terms = model(in1, in0, retPerLayer=True)
    assert torch.equal(ab, ba) and all(torch.equal(a, b) for a, b in zip(ab_terms, ba_terms)) and float(ab) > 0.1


def test_repeatable_and_batched(model):
    a0, a1 = (t.to(DEV) for t in lc.case("37x50"))
    g = torch.Generator().manual_seed(5)
    b0, b1 = torch.rand((1, 3, 37, 50), generator=g).to(DEV), torch.rand((1, 3, 37, 50), generator=g).to(DEV)
    in0, in1 = torch.cat([a0, b0]), torch.cat([a1, b1])
    keep0, keep1 = in0.clone(), in1.clone()
    first, first_terms = model(in0, in1, retPerLayer=True)
    again, again_terms = model(in0, in1, retPerLayer=True)
    assert first.shape == (2, 1, 1, 1) and torch.equal(first, again)
    assert all(torch.equal(a, b) for a, b in zip(first_terms, again_terms))
    for i, (x, y) in enumerate(((a0, a1), (b0, b1))):
        one, one_terms = model(x, y, retPerLayer=True)
        assert torch.equal(one[0], first[i]), i
        assert all(torch.equal(t[0], ft[i]) for t, ft in zip(one_terms, first_terms)), i
    assert torch.equal(model(a0[0], a1[0]), model(a0, a1)), "(3, h, w) is (1, 3, h, w)"
    feats = model.features(in0)
    assert all(torch.equal(f[:1], s) for f, s in zip(feats, model.features(a0)))
    assert torch.equal(in0, keep0) and torch.equal(in1, keep1)
    # nothing is read back on the way
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        model(in0, in1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


# ---- evaluate_views (the tiny renderer of tests/test_metrics_gpu.py's end-to-end test, built the same way) ------------------------
def tiny_view(human, layer, view, H=64, W=64):
    from humanliff_amd.SynBodyView_datasets import camera_rays
    K, c2w, cam = syn.orbit_camera(view, 8, H, W)
    R = c2w.T
    ro, rd, near, far, mask = camera_rays(H, W, K, R, -R @ cam, syn.WORLD_BOUNDS, DEV, return_mask=True)
    return {"ray_o_all": ro[None, None], "ray_d_all": rd[None, None], "near_all": near[None, None, :, None], "far_all": far[None, None, :, None],
            "mask_at_box_all": mask[None, None], "instance_idx": torch.tensor([human]), "cloth_layer_index": torch.tensor([layer]),
            "pose_index": torch.tensor([3]), "world_bounds": torch.tensor(syn.WORLD_BOUNDS)[None], "view_id": 145 + view}


def test_evaluate_views_fills_lpips(model, tmp_path):
    from humanliff_amd.recon_NeRF import Renderer
    from humanliff_amd.recon_NeRF.lib import all_test
    torch.manual_seed(0)
    r = Renderer(use_canonical_space=False, num_instances=2, triplane_dim=32, triplane_ch=27, test=True)
    r.load_state_dict(syn.render_mlp_state(3), strict=False)
    r = r.to(DEV)
    kw = dict(n_samples=16, n_importance=16)
    views, g = [], torch.Generator().manual_seed(4)
    for human in (0, 1):
        for view in (1, 5):
            tp = tiny_view(human, (human + view) % 4, view)
            own = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in tp.items()}
            rgb = all_test.render(chunk=256, rays_o=own["ray_o_all"][:, 0], rays_d=own["ray_d_all"][:, 0], near=own["near_all"][:, 0],
                                  far=own["far_all"][:, 0], tp_input=own, renderer=r, perturb=0., **kw)[0]
            noise = (torch.rand(rgb.shape, generator=g) - 0.5) * 0.1
            tp["rgb_all"] = (rgb.detach().cpu() + noise)[:, None]             # the renderer's own view plus known noise
            views.append(tp)
    crops = []

    def hook(a, b):
        crops.append((a, b))
        return model(a, b)

    def run(lpips_fn):
        torch.manual_seed(7)          # the importance samples' uniforms come from torch's CPU generator: the same renders every time
        return all_test.evaluate_views(r, views, lpips_fn=lpips_fn, **kw)

    metric, plain, direct = run(hook), run(None), run(model)
    got = metric["novel_view_lpips"]
    assert got.shape == (2, 2, 1) and np.isfinite(got).all() and (got > 0).all() and len(crops) == 4
    assert np.array_equal(got, direct["novel_view_lpips"]) and np.isnan(plain["novel_view_lpips"]).all()
    # evaluate_views_lpips: the same dict, lines' values and files, the scores read back once per subject
    from humanliff_amd.recon_NeRF.lib.lpips_views import evaluate_views_lpips
    torch.manual_seed(7)
    once = evaluate_views_lpips(r, views, model, savedir=str(tmp_path), **kw)
    for k in metric:
        assert np.array_equal(np.asarray(once[k]), np.asarray(metric[k])), k
    back = np.load(tmp_path / "metrics.npy", allow_pickle=True).item()
    assert np.array_equal(back["novel_view_lpips"], got)
    with open(tmp_path / "metrics.json") as f:
        assert json.load(f)["novel_view_all_human"][3] == metric["novel_view_all_human"][3].tolist()
    torch.manual_seed(7)
    floats = evaluate_views_lpips(r, views, lambda a, b: 0.25, **kw)          # a hook of Python floats passes through
    assert (floats["novel_view_lpips"] == 0.25).all()
    torch.manual_seed(7)
    none = evaluate_views_lpips(r, views, None, **kw)
    assert np.isnan(none["novel_view_lpips"]).all() and np.array_equal(none["novel_view_ssim"], plain["novel_view_ssim"])
    for i, (a, b) in enumerate(crops):
        assert a.shape[0] == 3 and min(a.shape[1:]) >= 16
        assert got[i // 2, i % 2, 0] == float(model(a, b)), i
    for k in ("mse", "psnr", "ssim"):
        assert np.array_equal(metric[f"novel_view_{k}"], plain[f"novel_view_{k}"]), k
    assert metric["novel_view_all_human"].shape == (4, 2) and np.isfinite(metric["novel_view_all_human"]).all()


def test_scores_of_a_subject_are_read_back_once(model):
    """Scoring a subject's views enqueues the hook for each of them without a sync; one copy then brings all the scores."""
    from humanliff_amd import metrics
    from humanliff_amd.recon_NeRF.lib import lpips_views
    g = torch.Generator().manual_seed(9)
    entries = []
    for v in range(3):
        pred, gt = (torch.rand((1, 40, 48, 3), generator=g).to(DEV) for _ in range(2))
        mask = torch.zeros((1, 40, 48), dtype=torch.bool, device=DEV)
        mask[:, 5:30 + v, 7 + v:40] = True                                    # a different crop per view
        entries.append({"rec": metrics.image_records(pred, gt, mask)[0], "batch": 1, "pred": pred, "gt": gt, "mask": mask})
    sub = {"entries": entries}
    rec = metrics.records_to_host(torch.cat([e["rec"] for e in entries]))
    want = []
    for v, e in enumerate(entries):
        x, y, w, h = (int(t) for t in rec["bbox"][v])
        assert (x, y, w, h) == (7 + v, 5, 33 - v, 25 + v)
        m = e["mask"][0, y:y + h, x:x + w, None]
        want.append(float(model((e["pred"][0, y:y + h, x:x + w] * m).permute(2, 0, 1), (e["gt"][0, y:y + h, x:x + w] * m).permute(2, 0, 1))))
    calls = []

    def hook(a, b):
        calls.append(a.shape)
        return model(a, b)

    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        scores, pending = lpips_views._enqueue_lpips(sub, rec, hook)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(calls) == 3 and [row for row, _ in pending] == [0, 1, 2] and all(np.isnan(scores))
    assert lpips_views._lpips_scores(sub, rec, model) == want
    assert lpips_views._lpips_scores(sub, rec, lambda a, b: torch.tensor([0.5])) == [0.5, 0.5, 0.5]
    assert all(np.isnan(lpips_views._lpips_scores(sub, rec, None)))
