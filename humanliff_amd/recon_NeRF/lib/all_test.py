"""The reference's test mode (recon_NeRF/run_nerf_batch.py --test -> recon_NeRF/lib/all_test.py test_SynBody / test_TightCap) without
its dataset classes: render held-out views, score them on the device (humanliff_amd.metrics), aggregate and save like the reference.

What differs from the reference, on purpose:
  * the views come from the caller (an iterable of tp_input dicts with the reference's keys), not from SynBodyDatasetBatch;
  * MSE, PSNR and SSIM are computed by hl_image_metrics on the device and read back once per subject, not once per view;
  * LPIPS needs the VGG weights of the `lpips` package, which are not available offline: no perceptual network is built here.
    `lpips_fn(pred_crop, gt_crop)` is a hook that receives what the reference hands to loss_fn_vgg; without it the entries are NaN;
  * the image pairs are saved as .npy (uint8, H x W x 3) under the reference's file stems: no PNG encoder is required.
"""
import json
import math
import os

import numpy as np
import torch

from ... import metrics as _metrics
from ..run_nerf_batch import render

VIEWS_PER_LAYER = 185       # the only views_num for which the reference defines its held-out list


def heldout_view_ids(views_num, test_layer_id=None, tightcap=False, view_ids=None):
    """view_id_lst of test_SynBody (all_test.py:100-109) or, with tightcap=True, of test_TightCap (:283-292): indices into the
    subject's 4 x views_num views (cloth layer = id // views_num).  Without test_layer_id two views per layer; with it the reference's
    range(145, 186) shifted by the layer - 41 ids, the last of which is view 0 of the NEXT layer (185 + 185 k), as in the reference.
    For views_num != 185 the reference leaves the list undefined (a NameError): ValueError here, unless the caller passes view_ids."""
    if view_ids is not None:
        return [int(i) for i in view_ids]
    if views_num != VIEWS_PER_LAYER:
        raise ValueError(f"the reference defines its held-out views for views_num == {VIEWS_PER_LAYER} only (got {views_num}): pass view_ids")
    a, b = (53, 146) if tightcap else (145, 165)
    view_id_lst = [a, b] + [a + views_num, b + views_num] + [a + views_num * 2, b + views_num * 2] + [a + views_num * 3, b + views_num * 3]
    if test_layer_id in (0, 1, 2, 3):
        view_id_lst = [i + test_layer_id * 185 for i in range(145, 186)]
    return view_id_lst


def aggregate(all_human_mse, all_human_psnr, all_human_ssim, all_human_lpips, human_names=()):
    """The reference's `metric` dict (:67-71, 207-218) from the nested lists human x pose x view (the reference's names for its loops:
    one `pose` entry per tp_input it scores, one `view` entry per batch element of it)."""
    metric = {
        "novel_view_mean_human": [], "novel_view_all_human": [], "novel_view_mse": [], "novel_view_psnr": [], "novel_view_ssim": [], "novel_view_lipis": [],
        "novel_pose_mean_human": [], "novel_pose_all_human": [], "novel_pose_mse": [], "novel_pose_psnr": [], "novel_pose_ssim": [], "novel_pose_lpips": [],
        "all_human_names": list(human_names),
    }
    human_num = len(all_human_psnr)
    metric["novel_view_mse"] = np.array(all_human_mse)
    metric["novel_view_psnr"] = np.array(all_human_psnr)
    metric["novel_view_ssim"] = np.array(all_human_ssim)
    metric["novel_view_lpips"] = np.array(all_human_lpips)
    metric["novel_view_mean_human"] = np.array([np.mean(metric["novel_view_mse"][:, :, :]), np.mean(metric["novel_view_psnr"][:, :, :]), np.mean(metric["novel_view_ssim"][:, :, :])])
    metric["novel_view_all_human"] = np.array([
        np.mean(metric["novel_view_mse"][:, :, :].reshape(human_num, -1), axis=-1),
        np.mean(metric["novel_view_psnr"][:, :, :].reshape(human_num, -1), axis=-1),
        np.mean(metric["novel_view_ssim"][:, :, :].reshape(human_num, -1), axis=-1),
        np.mean(metric["novel_view_lpips"][:, :, :].reshape(human_num, -1), axis=-1),
    ])
    return metric


def save_metric(metric, savedir):
    """metrics.json (the two summary arrays) and metrics.npy (the whole dict, pickled by np.save), :220-227."""
    os.makedirs(savedir, exist_ok=True)
    metric_json = {}
    with open(os.path.join(savedir, "metrics.json"), 'w') as f:
        metric_json["novel_view_mean_human"] = metric["novel_view_mean_human"].tolist()
        metric_json["novel_view_all_human"] = metric["novel_view_all_human"].tolist()
        json.dump(metric_json, f)
    np.save(os.path.join(savedir, "metrics.npy"), metric)


def _image_size(tp_input, n_rays):
    if "H" in tp_input and "W" in tp_input:
        H, W = int(tp_input["H"]), int(tp_input["W"])
    else:                                       # the reference's views are square (H = W = int(1024 * image_scaling), :52)
        H = W = math.isqrt(n_rays)
    if H * W != n_rays:
        raise ValueError(f"a view of {n_rays} rays is not {H} x {W}: give tp_input['H'] and tp_input['W']")
    return H, W


def _index(t):
    return int(t.reshape(-1)[0]) if torch.is_tensor(t) else int(t)


def _finish_subject(sub, lpips_fn, savedir):
    """One read-back for all the subject's views; the [Test] lines, the files and the subject's pose x view lists."""
    rec = _metrics.records_to_host(torch.cat([e["rec"] for e in sub["entries"]]))
    if savedir is not None:
        save_path = os.path.join(savedir, "novel_view", sub["name"])
        os.makedirs(save_path, exist_ok=True)
    lists = {k: [] for k in ("mse", "psnr", "ssim", "lpips")}
    row = 0
    for e in sub["entries"]:
        per = {k: [] for k in lists}
        for key in ("layer", "pose"):
            e[key] = [int(v) for v in torch.as_tensor(e[key]).reshape(-1).expand(e["batch"]).tolist()]
        for j in range(e["batch"]):
            mse, psnr, ssim = float(rec["mse"][row]), float(rec["psnr"][row]), float(rec["ssim"][row])
            lpips = float("nan")
            if lpips_fn is not None:
                x, y, w, h = (int(v) for v in rec["bbox"][row])
                m = e["mask"][j, y:y + h, x:x + w, None]
                pred_crop = (e["pred"][j, y:y + h, x:x + w] * m).permute(2, 0, 1).contiguous()
                gt_crop = (e["gt"][j, y:y + h, x:x + w] * m).permute(2, 0, 1).contiguous()
                out = lpips_fn(pred_crop, gt_crop)
                lpips = float(out.reshape(-1)[0]) if torch.is_tensor(out) else float(out)
            if savedir is not None:
                stem = 'cloth_layer{:04d}_frame{:04d}_view{:04d}'.format(e["layer"][j], e["pose"][j], e["view_id"])
                np.save(os.path.join(save_path, stem + "_gt.npy"), e["gt_u8"][j].cpu().numpy())
                np.save(os.path.join(save_path, stem + ".npy"), e["pred_u8"][j].cpu().numpy())
            print("[Test] ", "human: ", sub["name"], " cloth_layer:", e["layer"][j], " pose:", e["pose"][j], " view:", e["view_id"],
                  " mse:", round(mse, 5), " psnr:", {psnr}, " ssim:", {ssim}, " lpips:", {lpips})
            for k, val in (("mse", mse), ("psnr", psnr), ("ssim", ssim), ("lpips", lpips)):
                per[k].append(val)
            row += 1
        for k in lists:
            lists[k].append(per[k])
    return lists


def evaluate_views(renderer, views, *, n_samples=128, n_importance=128, white_bkgd=False, data_range=_metrics.REFERENCE_DATA_RANGE,
                   lpips_fn=None, savedir=None, human_names=None):
    """test_SynBody's loop (:116-205) over `views`, an iterable of tp_input dicts with the reference's keys: ray_o_all, ray_d_all,
    near_all, far_all, rgb_all, mask_at_box_all (batch, views, rays, .; index k = 0 is rendered, as in the reference), instance_idx,
    cloth_layer_index, pose_index and whatever the renderer reads (world_bounds).  Optional keys: H and W (else the view is square)
    and view_id (else the view's position among its subject's views).  Consecutive views of one instance_idx form a subject; every
    subject must bring the same number of views.  `renderer` holds the fitted tri-planes (recon_NeRF.Renderer, test=True) on the device.

    Returns the reference's `metric` dict (see aggregate); with `savedir` also writes metrics.json, metrics.npy and, under
    novel_view/<human>/, the uint8 prediction / ground-truth pairs as .npy with the reference's file stems."""
    core = renderer.module if hasattr(renderer, "module") else renderer
    dev = core.tri_planes.device
    if dev.type != "cuda":
        raise RuntimeError("evaluate_views needs the Renderer on a HIP device; humanliff_amd has no CPU path")
    subjects, sub = [], None
    per_human = {k: [] for k in ("mse", "psnr", "ssim", "lpips")}

    def close():
        lists = _finish_subject(sub, lpips_fn, savedir)
        for k in per_human:
            per_human[k].append(lists[k])

    for tp_input in views:
        human_id = _index(tp_input['instance_idx'])
        if sub is None or sub["human_id"] != human_id:
            if sub is not None:
                close()
            name = str(human_names[human_id]).strip() if human_names is not None else '{:04d}'.format(human_id)
            sub = {"human_id": human_id, "name": name, "entries": []}
            subjects.append(name)
        tp_input = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in tp_input.items()}
        k = 0
        rays_o = tp_input['ray_o_all'][:, k]
        rays_d = tp_input['ray_d_all'][:, k]
        near = tp_input['near_all'][:, k]
        far = tp_input['far_all'][:, k]
        target_s = tp_input['rgb_all'][:, k]
        mask_at_box = tp_input['mask_at_box_all'][:, k]
        batch_size, n_rays = rays_d.shape[0], rays_d.shape[1]
        H, W = _image_size(tp_input, n_rays)
        with torch.no_grad():
            rgb, acc, normal_map, depth_map = render(chunk=max(H * W // 16, 1), rays_o=rays_o, rays_d=rays_d, tp_input=tp_input, near=near, far=far,
                                                     renderer=renderer, n_samples=n_samples, perturb=0., n_importance=n_importance,
                                                     white_bkgd=white_bkgd)
        rgb = rgb.reshape(batch_size, H, W, 3).detach().float()
        target_s = target_s.reshape(batch_size, H, W, 3).float()
        mask_at_box = mask_at_box.reshape(batch_size, H, W)
        if mask_at_box.dtype not in (torch.bool, torch.uint8):
            mask_at_box = mask_at_box != 0
        rec, pred_u8, gt_u8 = _metrics.image_records(rgb, target_s, mask_at_box, data_range, return_uint8=savedir is not None)
        entry = {"rec": rec, "batch": batch_size, "view_id": int(tp_input.get("view_id", len(sub["entries"]))),
                 "layer": tp_input['cloth_layer_index'], "pose": tp_input.get('pose_index', 0),      # (read with the records, not here)
                 "pred_u8": pred_u8, "gt_u8": gt_u8}
        if lpips_fn is not None:
            entry.update(pred=rgb, gt=target_s, mask=mask_at_box != 0)
        sub["entries"].append(entry)
    if sub is None:
        raise ValueError("evaluate_views: no views")
    close()
    metric = aggregate(per_human["mse"], per_human["psnr"], per_human["ssim"], per_human["lpips"], subjects)
    if savedir is not None:
        save_metric(metric, savedir)
    return metric
