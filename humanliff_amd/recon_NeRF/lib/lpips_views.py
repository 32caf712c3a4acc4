"""Held-out view evaluation with the perceptual score kept on the device: all_test.evaluate_views' loop with one change - what the
LPIPS hook returns as device tensors (humanliff_amd.lpips.LpipsVGG does) is collected for all of a subject's views and read back in
one copy with the subject's records, instead of one float() sync per view.  Everything else - rendering, records, [Test] lines,
files, the `metric` dict - is all_test's, through its own helpers; hooks that return Python floats or host tensors behave as there.

Why this is a module of its own: all_test.py carries the reference's file name, which the project's rules read as a test file, and
existing test files are frozen for feature changes.  all_test.evaluate_views is therefore left as it is (an LpipsVGG works as its
lpips_fn too, at one sync per view, with the same numbers); this is the entry point for scoring with LPIPS.  Contract: DESIGN.md 4f.
"""
import os

import numpy as np
import torch

from ... import metrics as _metrics
from . import all_test
from .all_test import _image_size, _index, aggregate, save_metric


def _enqueue_lpips(sub, rec, lpips_fn):
    """lpips_fn on every view's masked crops, in view order.  Returns (scores, pending): a Python float per view (NaN where the value is
    still on the device, or without the hook) and (row, (1,) float64 device tensor) for those.  Nothing is read back here."""
    scores, pending = [], []
    for e in sub["entries"]:
        for j in range(e["batch"]):
            row = len(scores)
            scores.append(float("nan"))
            if lpips_fn is None:
                continue
            x, y, w, h = (int(v) for v in rec["bbox"][row])
            m = e["mask"][j, y:y + h, x:x + w, None]
            pred_crop = (e["pred"][j, y:y + h, x:x + w] * m).permute(2, 0, 1).contiguous()
            gt_crop = (e["gt"][j, y:y + h, x:x + w] * m).permute(2, 0, 1).contiguous()
            out = lpips_fn(pred_crop, gt_crop)
            if torch.is_tensor(out) and out.is_cuda:
                pending.append((row, out.detach().reshape(-1)[:1].double()))        # (float32 -> float64 is exact)
            else:
                scores[row] = float(out.reshape(-1)[0]) if torch.is_tensor(out) else float(out)
    return scores, pending


def _lpips_scores(sub, rec, lpips_fn):
    """The subject's scores as Python floats: every view enqueued, then one copy to the host."""
    scores, pending = _enqueue_lpips(sub, rec, lpips_fn)
    if pending:
        for (row, _), val in zip(pending, torch.cat([t for _, t in pending]).cpu().tolist()):
            scores[row] = val
    return scores


def _finish_subject(sub, lpips_fn, savedir):
    """all_test._finish_subject with the hook's results read back once: the records, then the scores, then the lines and files."""
    rec = _metrics.records_to_host(torch.cat([e["rec"] for e in sub["entries"]]))
    scores = _lpips_scores(sub, rec, lpips_fn)
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
            mse, psnr, ssim, lpips = float(rec["mse"][row]), float(rec["psnr"][row]), float(rec["ssim"][row]), scores[row]
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


def evaluate_views_lpips(renderer, views, lpips_fn, *, n_samples=128, n_importance=128, white_bkgd=False,
                         data_range=_metrics.REFERENCE_DATA_RANGE, savedir=None, human_names=None):
    """all_test.evaluate_views(renderer, views, lpips_fn=lpips_fn, ...) - same arguments, same `metric` dict, lines and files - with the
    hook's device results read back once per subject."""
    core = renderer.module if hasattr(renderer, "module") else renderer
    dev = core.tri_planes.device
    if dev.type != "cuda":
        raise RuntimeError("evaluate_views_lpips needs the Renderer on a HIP device; humanliff_amd has no CPU path")
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
        rays_o, rays_d = tp_input['ray_o_all'][:, 0], tp_input['ray_d_all'][:, 0]          # (index k = 0 is rendered, as in the reference)
        near, far = tp_input['near_all'][:, 0], tp_input['far_all'][:, 0]
        target_s, mask_at_box = tp_input['rgb_all'][:, 0], tp_input['mask_at_box_all'][:, 0]
        batch_size, n_rays = rays_d.shape[0], rays_d.shape[1]
        H, W = _image_size(tp_input, n_rays)
        with torch.no_grad():
            rgb = all_test.render(chunk=max(H * W // 16, 1), rays_o=rays_o, rays_d=rays_d, tp_input=tp_input, near=near, far=far,
                                  renderer=renderer, n_samples=n_samples, perturb=0., n_importance=n_importance, white_bkgd=white_bkgd)[0]
        rgb = rgb.reshape(batch_size, H, W, 3).detach().float()
        target_s = target_s.reshape(batch_size, H, W, 3).float()
        mask_at_box = mask_at_box.reshape(batch_size, H, W)
        if mask_at_box.dtype not in (torch.bool, torch.uint8):
            mask_at_box = mask_at_box != 0
        rec, pred_u8, gt_u8 = _metrics.image_records(rgb, target_s, mask_at_box, data_range, return_uint8=savedir is not None)
        entry = {"rec": rec, "batch": batch_size, "view_id": int(tp_input.get("view_id", len(sub["entries"]))),
                 "layer": tp_input['cloth_layer_index'], "pose": tp_input.get('pose_index', 0), "pred_u8": pred_u8, "gt_u8": gt_u8}
        if lpips_fn is not None:
            entry.update(pred=rgb, gt=target_s, mask=mask_at_box != 0)
        sub["entries"].append(entry)
    if sub is None:
        raise ValueError("evaluate_views_lpips: no views")
    close()
    metric = aggregate(per_human["mse"], per_human["psnr"], per_human["ssim"], per_human["lpips"], subjects)
    if savedir is not None:
        save_metric(metric, savedir)
    return metric
