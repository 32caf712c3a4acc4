"""hl_image_metrics on the MI355X (humanliff_amd/metrics.py, csrc/hl_metrics.hip) against the float64 restatement of the reference's
psnr_metric / ssim_metric (tests/metrics_restatement.py), and evaluate_views (recon_NeRF/lib/all_test.py) end to end on a tiny renderer.

Bounds (tests/metrics_cases.py): count, the box and the uint8 images are exact; ssim is within 100 x the restatement's own
summation-order noise (capped at 1e-10 absolute), mse within 100 x (capped at 1e-12 relative), psnr within what that mse bound and
the roundings of its expression allow."""
import json
import os

import numpy as np
import pytest
import torch

from humanliff_amd import metrics
from humanliff_amd import synthetic as syn
from tests import metrics_cases as mc
from tests import metrics_restatement as mr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def to_dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def check_view(got, v, want, tag):
    ssim_bound, mse_bound = mc.device_bounds()
    mse, psnr, ssim = float(got["mse"][v]), float(got["psnr"][v]), float(got["ssim"][v])
    e_mse, e_psnr, e_ssim = abs(mse - want["mse"]) / want["mse"], abs(psnr - want["psnr"]), abs(ssim - want["ssim"])
    print(f"{tag}: mse {mse!r} relative error {e_mse:.3e} (bound {mse_bound:.1e}); psnr {psnr!r} error {e_psnr:.3e} "
          f"(bound {mc.psnr_bound(want['psnr'], mse_bound):.1e}); ssim {ssim!r} error {e_ssim:.3e} (bound {ssim_bound:.1e})")
    assert int(got["count"][v]) == want["count"], tag
    assert tuple(int(t) for t in got["bbox"][v]) == want["bbox"], tag
    assert e_mse <= mse_bound, tag
    assert e_psnr <= mc.psnr_bound(want["psnr"], mse_bound), tag
    assert e_ssim <= ssim_bound, tag


@pytest.mark.parametrize("name", list(mc.CASES))
def test_one_view_matches_the_restatement(name):
    pred, gt, mask, want_box = mc.case(name)
    want = mc.reference(name)
    assert want["bbox"] == want_box
    p, g, m = to_dev(pred, gt, mask)
    p0, g0 = p.clone(), g.clone()
    got = metrics.image_metrics(p, g, m, return_uint8=True)
    assert all(got[k].is_cuda for k in got) and got["mse"].dtype == torch.float64 and got["bbox"].dtype == torch.int32
    assert got["mse"].shape == (1,) and got["bbox"].shape == (1, 4) and got["pred_u8"].shape == (1,) + pred.shape
    host = {k: t.cpu().numpy() for k, t in got.items()}
    check_view(host, 0, want, name)
    assert np.array_equal(host["pred_u8"][0], want["pred_u8"]) and np.array_equal(host["gt_u8"][0], want["gt_u8"])
    assert torch.equal(p, p0) and torch.equal(g, g0), "pred and gt are only read"
    # the reference's own float32 psnr_metric: within float32 rounding of ours.  np.mean's float32 sum of n terms (pairwise above
    # blocks of 128, 8 accumulators of 16 sequential terms within one) is good to (log2(n) + 16) eps relative at the worst, each square
    # to one eps; a relative error e of mse moves psnr by 10 e / ln 10, and the float32 logarithm, product and quotient of
    # the expression add a few eps of the value
    n = 3 * want["count"]
    eps = float(np.finfo(np.float32).eps)
    bound32 = 10.0 / np.log(10.0) * (np.log2(n) + 17) * eps + 4 * eps * abs(want["psnr"])
    ref32 = mr.psnr_float32(*mr.masked_values(pred, gt, mask))
    print(f"{name}: float32 psnr_metric {ref32!r}, ours {float(host['psnr'][0])!r}, difference {abs(ref32 - host['psnr'][0]):.3e} (bound {bound32:.1e})")
    assert abs(ref32 - float(host["psnr"][0])) <= bound32
    # a second run gives the same bits; a uint8 mask and the (H, W, 3) form give the same record
    again = metrics.image_metrics(p, g, m.to(torch.uint8) * 255)
    stacked = metrics.image_metrics(p[None], g[None], m[None])
    for k in ("mse", "psnr", "ssim", "count", "bbox"):
        assert torch.equal(again[k], got[k]) and torch.equal(stacked[k], got[k]), k


def three_views():
    """Three 37 x 53 views with different boxes, stacked."""
    names = ("23x39", "7x7", "borders")
    pred, gt, mask = (np.stack([mc.case(n)[i] for n in names]) for i in range(3))
    return names, pred, gt, mask


def test_three_views_equal_three_calls_bit_for_bit():
    names, pred, gt, mask = three_views()
    p, g, m = to_dev(pred, gt, mask)
    got = metrics.image_metrics(p, g, m, return_uint8=True)
    host = metrics.image_metrics_host(p, g, m)
    for v, name in enumerate(names):
        check_view(host, v, mc.reference(name), f"view {v} ({name})")
        one = metrics.image_metrics(p[v], g[v], m[v], return_uint8=True)
        for k in one:
            assert torch.equal(one[k][0], got[k][v]), (name, k)
        assert host["mse"][v] == float(got["mse"][v]) and host["ssim"][v] == float(got["ssim"][v])


def test_degenerate_crops():
    pred, gt, mask, want_box = mc.make(*mc.SMALL, seed=3)
    p, g, m = to_dev(pred, gt, mask)
    got = metrics.image_metrics(p, g, m)
    assert tuple(got["bbox"][0].tolist()) == want_box and want_box[2:] == (9, 6)
    assert bool(torch.isnan(got["ssim"][0])) and float(got["mse"][0]) > 0 and int(got["count"][0]) == int(mask.sum())
    want_mse, want_psnr = mr.mse_psnr(*mr.masked_values(pred, gt, mask))
    assert abs(float(got["mse"][0]) - want_mse) <= mc.device_bounds()[1] * want_mse
    with pytest.raises(ValueError, match="view 0"):
        metrics.image_metrics_host(p, g, m)
    # an empty mask: a (0, 0, 0, 0) box, nothing counted, every score NaN
    empty = torch.zeros_like(m)
    got = metrics.image_metrics(p, g, empty, return_uint8=True)
    assert got["bbox"][0].tolist() == [0, 0, 0, 0] and int(got["count"][0]) == 0
    assert all(bool(torch.isnan(got[k][0])) for k in ("mse", "psnr", "ssim"))
    assert not bool(got["pred_u8"].any()) and np.array_equal(got["gt_u8"][0].cpu().numpy(), mr.to8b(gt))
    with pytest.raises(ValueError, match="view 1"):
        metrics.image_metrics_host(torch.stack([p, p]), torch.stack([g, g]), torch.stack([torch.ones_like(m), empty]))
    # images smaller than the window
    tiny = metrics.image_metrics(p[:5, :4], g[:5, :4], torch.ones((5, 4), dtype=torch.bool, device=DEV))
    assert tiny["bbox"][0].tolist() == [0, 0, 4, 5] and bool(torch.isnan(tiny["ssim"][0])) and float(tiny["mse"][0]) > 0


def test_nan_stays_in_its_view():
    names, pred, gt, mask = three_views()
    p, g, m = to_dev(pred, gt, mask)
    clean = metrics.image_metrics(p, g, m)
    x, y, w, h = mc.reference(names[1])["bbox"]
    assert bool(m[1, y, x])
    p[1, y, x, 1] = float("nan")
    got = metrics.image_metrics(p, g, m)
    for k in ("mse", "psnr", "ssim"):
        assert bool(torch.isnan(got[k][1])), k
        assert torch.equal(got[k][[0, 2]], clean[k][[0, 2]]), k
    assert torch.equal(got["bbox"], clean["bbox"]) and torch.equal(got["count"], clean["count"])
    # a NaN outside the mask is not seen at all
    p[1, y, x, 1] = clean_value = float(pred[1, y, x, 1])
    outside = torch.nonzero(~m[0])[0]
    p[0, outside[0], outside[1], 2] = float("nan")
    got = metrics.image_metrics(p, g, m)
    for k in ("mse", "psnr", "ssim"):
        assert torch.equal(got[k], clean[k]), (k, clean_value)


def test_arguments():
    pred, gt, mask, _ = mc.case("23x39")
    p, g, m = to_dev(pred, gt, mask)
    for bad in ((p.cpu(), g, m), (p, g.cpu(), m), (p, g, m.cpu())):
        with pytest.raises(RuntimeError):
            metrics.image_metrics(*bad)
    with pytest.raises(RuntimeError):
        metrics.image_metrics(p.double(), g.double(), m)
    with pytest.raises(RuntimeError):
        metrics.image_metrics(p, g, m[:-1])
    # data_range is skimage's R: it moves ssim only
    r2, r1 = metrics.image_metrics(p, g, m), metrics.image_metrics(p, g, m, data_range=1.0)
    want = mc.reference("23x39", 1.0)
    assert abs(float(r1["ssim"][0]) - want["ssim"]) <= mc.device_bounds()[0]
    assert abs(want["ssim"] - mc.reference("23x39")["ssim"]) > 1e-3 and float(r1["ssim"][0]) != float(r2["ssim"][0])
    assert torch.equal(r1["mse"], r2["mse"]) and torch.equal(r1["psnr"], r2["psnr"])
    # nothing is read back on the way
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        metrics.image_metrics(p, g, m, return_uint8=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


# ---- evaluate_views ---------------------------------------------------------------------------------------------------------------
def tiny_view(human, layer, view, H=32, W=32):
    from humanliff_amd.SynBodyView_datasets import camera_rays
    K, c2w, cam = syn.orbit_camera(view, 8, H, W)
    R = c2w.T
    ro, rd, near, far, mask = camera_rays(H, W, K, R, -R @ cam, syn.WORLD_BOUNDS, DEV, return_mask=True)
    return {"ray_o_all": ro[None, None], "ray_d_all": rd[None, None], "near_all": near[None, None, :, None], "far_all": far[None, None, :, None],
            "mask_at_box_all": mask[None, None], "instance_idx": torch.tensor([human]), "cloth_layer_index": torch.tensor([layer]),
            "pose_index": torch.tensor([3]), "world_bounds": torch.tensor(syn.WORLD_BOUNDS)[None], "view_id": 145 + view}


def test_evaluate_views_end_to_end(tmp_path, monkeypatch):
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
            assert int(tp["mask_at_box_all"].sum()) > 49
            own = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in tp.items()}
            rgb = all_test.render(chunk=64, rays_o=own["ray_o_all"][:, 0], rays_d=own["ray_d_all"][:, 0], near=own["near_all"][:, 0],
                                  far=own["far_all"][:, 0], tp_input=own, renderer=r, perturb=0., **kw)[0]
            noise = (torch.rand(rgb.shape, generator=g) - 0.5) * 0.1
            tp["rgb_all"] = (rgb.detach().cpu() + noise)[:, None]             # the renderer's own view plus known noise
            views.append(tp)
    rendered = []
    render = all_test.render

    def recording(**k):
        out = render(**k)
        rendered.append(out[0].detach().clone())
        return out

    monkeypatch.setattr(all_test, "render", recording)
    crops = []
    metric = all_test.evaluate_views(r, views, savedir=str(tmp_path), human_names=["anna", "ben"],
                                     lpips_fn=lambda a, b: crops.append((a, b)) or torch.tensor([0.25]), **kw)
    assert len(rendered) == 4 and len(crops) == 4
    for k in ("mse", "psnr", "ssim", "lpips"):
        assert metric[f"novel_view_{k}"].shape == (2, 2, 1), k
    assert metric["all_human_names"] == ["anna", "ben"] and (metric["novel_view_lpips"] == 0.25).all()
    ssim_bound, mse_bound = mc.device_bounds()
    for i, tp in enumerate(views):
        pred = rendered[i].reshape(32, 32, 3).cpu().numpy()
        gt = tp["rgb_all"].reshape(32, 32, 3).numpy()
        mask = tp["mask_at_box_all"].reshape(32, 32).cpu().numpy()
        want = mr.view_metrics(pred, gt, mask)
        got = {k: metric[f"novel_view_{k}"][i // 2, i % 2, 0] for k in ("mse", "psnr", "ssim")}
        print(f"view {i}: mse {got['mse']!r} restatement {want['mse']!r}; ssim {got['ssim']!r} restatement {want['ssim']!r}")
        assert abs(got["mse"] - want["mse"]) <= mse_bound * want["mse"]
        assert abs(got["psnr"] - want["psnr"]) <= mc.psnr_bound(want["psnr"], mse_bound)
        assert abs(got["ssim"] - want["ssim"]) <= ssim_bound
        x, y, w, h = want["bbox"]
        assert crops[i][0].shape == (3, h, w) and crops[i][0].is_cuda and crops[i][0].dtype == torch.float32
        m3 = mask[y:y + h, x:x + w, None]
        assert np.array_equal(crops[i][0].permute(1, 2, 0).cpu().numpy(), pred[y:y + h, x:x + w] * m3)
        assert np.array_equal(crops[i][1].permute(1, 2, 0).cpu().numpy(), gt[y:y + h, x:x + w] * m3)
        stem = os.path.join(tmp_path, "novel_view", ["anna", "ben"][i // 2],
                            "cloth_layer{:04d}_frame0003_view{:04d}".format(int(tp["cloth_layer_index"]), tp["view_id"]))
        assert np.array_equal(np.load(stem + ".npy"), want["pred_u8"]) and np.array_equal(np.load(stem + "_gt.npy"), want["gt_u8"])
    with open(os.path.join(tmp_path, "metrics.json")) as f:
        js = json.load(f)
    assert list(js) == ["novel_view_mean_human", "novel_view_all_human"]
    assert len(js["novel_view_mean_human"]) == 3 and [len(row) for row in js["novel_view_all_human"]] == [2, 2, 2, 2]
    assert js["novel_view_mean_human"][0] == float(np.mean(metric["novel_view_mse"]))
    back = np.load(os.path.join(tmp_path, "metrics.npy"), allow_pickle=True).item()
    assert np.array_equal(back["novel_view_ssim"], metric["novel_view_ssim"])
    # without the hook no perceptual network is built: NaN
    monkeypatch.setattr(all_test, "render", render)
    plain = all_test.evaluate_views(r, views[:2], **kw)
    assert plain["novel_view_lpips"].shape == (1, 2, 1) and np.isnan(plain["novel_view_lpips"]).all()
