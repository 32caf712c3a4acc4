"""Float64 numpy / scipy restatement of the reference's per-view scores (recon_NeRF/lib/all_test.py): psnr_metric (:19-22), the bounding
rectangle cv2.boundingRect returns for a mask (:32), ssim_metric (:24-37) with skimage.metrics.structural_similarity's defaults, and
to8b.  This is the yardstick of tests/test_metrics_gpu.py.  skimage and cv2 are not importable where these tests run, so it restates
their documented behaviour line by line; agreement with the packages themselves is unverified (DESIGN.md "Evaluation").
"""
import numpy as np
from scipy.ndimage import uniform_filter

WIN_SIZE = 7


def to8b(x):
    """to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)"""
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def masked_values(img_pred, img_gt, mask_at_box):
    """img_pred[mask_at_box[j]], gt_img[mask_at_box[j]] (all_test.py:186-188): (count, 3) float32 each."""
    m = np.asarray(mask_at_box).astype(bool)
    return np.asarray(img_pred, dtype=np.float32)[m], np.asarray(img_gt, dtype=np.float32)[m]


def mse_psnr(rgb_pred, rgb_gt):
    """psnr_metric (:19-22) with the float32 difference the reference's tensors give and float64 from the squaring on:
           mse = np.mean((img_pred - img_gt)**2);  psnr = -10 * np.log(mse) / np.log(10)"""
    diff = (rgb_pred - rgb_gt).astype(np.float64)            # float32 - float32, then widened
    with np.errstate(all="ignore"):
        mse = np.mean(diff ** 2) if diff.size else np.float64("nan")
        psnr = -10 * np.log(mse) / np.log(10)
    return float(mse), float(psnr)


def psnr_float32(rgb_pred, rgb_gt):
    """psnr_metric exactly as the reference runs it: float32 arrays in, np.mean in float32."""
    mse = np.mean((rgb_pred - rgb_gt) ** 2)
    return float(-10 * np.log(mse) / np.log(10))


def bounding_rect(mask):
    """x, y, w, h = cv2.boundingRect(mask.astype(np.uint8)): the smallest upright rectangle holding every nonzero pixel, x / y its
    smallest column / row, w / h the largest minus the smallest plus one; (0, 0, 0, 0) for an empty mask."""
    ys, xs = np.nonzero(np.asarray(mask))
    if ys.size == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def box_filter_cumsum(a, size=WIN_SIZE):
    """Mean over size x size windows by cumulative sums (another summation order than uniform_filter's).  The value at an interior
    position equals uniform_filter's; border positions are left NaN: they are never counted."""
    H, W = a.shape
    c = np.zeros((H + 1, W + 1))
    c[1:, 1:] = np.cumsum(np.cumsum(a, axis=0), axis=1)
    s = c[size:, size:] - c[:-size, size:] - c[size:, :-size] + c[:-size, :-size]
    out = np.full((H, W), np.nan)
    r = size // 2
    out[r:H - r, r:W - r] = s / (size * size)
    return out


def _uniform(a, size=WIN_SIZE):
    return uniform_filter(a, size=size)


def structural_similarity_channel(im1, im2, data_range, filter_func=_uniform):
    """skimage.metrics.structural_similarity for one 2-D float64 channel with its defaults: win_size 7, uniform window,
    use_sample_covariance True, K1 0.01, K2 0.03."""
    win_size = WIN_SIZE
    if np.any((np.asarray(im1.shape) - win_size) < 0):
        raise ValueError("win_size exceeds image extent.")
    K1, K2 = 0.01, 0.03
    ndim = im1.ndim
    NP = win_size ** ndim
    cov_norm = NP / (NP - 1)                                # sample covariance
    ux = filter_func(im1)
    uy = filter_func(im2)
    uxx = filter_func(im1 * im1)
    uyy = filter_func(im2 * im2)
    uxy = filter_func(im1 * im2)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    R = data_range
    C1 = (K1 * R) ** 2
    C2 = (K2 * R) ** 2
    A1, A2, B1, B2 = (2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2)
    D = B1 * B2
    S = (A1 * A2) / D
    pad = (win_size - 1) // 2                                # to avoid edge effects will ignore filter radius strip around edges
    return S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean(dtype=np.float64)


def ssim_metric(rgb_pred, rgb_gt, mask_at_box, H, W, data_range=2.0, filter_func=_uniform):
    """ssim_metric (:24-37).  data_range: the reference passes float64 images and no data_range, for which the skimage of its pinned
    environment takes the dtype range of a float image, (-1, 1): 2."""
    mask_at_box = np.asarray(mask_at_box).astype(bool)
    # convert the pixels into an image
    img_pred = np.zeros((H, W, 3))
    img_pred[mask_at_box] = rgb_pred
    img_gt = np.zeros((H, W, 3))
    img_gt[mask_at_box] = rgb_gt
    # crop the object region
    x, y, w, h = bounding_rect(mask_at_box.astype(np.uint8))
    img_pred = img_pred[y:y + h, x:x + w]
    img_gt = img_gt[y:y + h, x:x + w]
    # compute the ssim: multichannel=True is the mean of the channels' values
    nch = img_pred.shape[-1]
    mssim = np.empty(nch)
    for ch in range(nch):
        mssim[ch] = structural_similarity_channel(img_pred[..., ch], img_gt[..., ch], data_range, filter_func)
    return float(mssim.mean())


def view_metrics(img_pred, img_gt, mask_at_box, data_range=2.0, filter_func=_uniform):
    """Everything the device record of one view holds, plus the two uint8 images the reference saves (:178-180)."""
    img_pred, img_gt = np.asarray(img_pred, dtype=np.float32), np.asarray(img_gt, dtype=np.float32)
    m = np.asarray(mask_at_box).astype(bool)
    H, W = m.shape
    rgb_pred, rgb_gt = masked_values(img_pred, img_gt, m)
    mse, psnr = mse_psnr(rgb_pred, rgb_gt)
    masked_pred = img_pred.copy()
    masked_pred[~m] = 0
    return {"mse": mse, "psnr": psnr, "ssim": ssim_metric(rgb_pred, rgb_gt, m, H, W, data_range, filter_func),
            "count": int(m.sum()), "bbox": bounding_rect(m), "pred_u8": to8b(masked_pred), "gt_u8": to8b(img_gt)}
