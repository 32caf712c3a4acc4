"""Float64 numpy restatement of the reference's training ray batches (recon_NeRF/lib/if_nerf_data_utils.py): project /
get_bound_corners (:20-39, 192-201), get_bound_2d_mask (:36-47) with the closed integer fill DESIGN.md 4g defines in place of
cv2.fillPoly, get_rays (:5-18), get_near_far (:50-85) and the split == 'train' loop of sample_ray_batch (:102-170) with the
np.random.randint draws handed in as `picks`.  This is the yardstick of tests/test_ray_batch_gpu.py; tests/test_ray_batch_cpu.py
pins it to tests/golden/ray_batch.npz, which the reference itself wrote.  cv2 is not importable where these tests run: fill_closed
is the rule the project defines, and tests/golden/gen_golden_ray_batch.py hands the same function to the reference as its fillPoly.
"""
import numpy as np

QUADS = [[0, 1, 3, 2], [4, 5, 7, 6], [0, 1, 5, 4], [2, 3, 7, 6], [0, 2, 6, 4], [1, 3, 7, 5]]     # get_bound_2d_mask :41-46


def bound_corners_2d(bounds, K, R, T):
    """np.round(project(get_bound_corners(bounds), K, [R|T])).astype(int): (8, 2) integer pixel coordinates (x, y)."""
    bounds = np.asarray(bounds)
    (min_x, min_y, min_z), (max_x, max_y, max_z) = bounds[0], bounds[1]
    corners_3d = np.array([[min_x, min_y, min_z], [min_x, min_y, max_z], [min_x, max_y, min_z], [min_x, max_y, max_z],
                           [max_x, min_y, min_z], [max_x, min_y, max_z], [max_x, max_y, min_z], [max_x, max_y, max_z]])
    RT = np.concatenate([np.asarray(R), np.asarray(T).reshape(3, 1)], axis=1)
    xyz = np.dot(corners_3d, RT[:, :3].T) + RT[:, 3:].T
    xyz = np.dot(xyz, np.asarray(K).T)
    xy = xyz[:, :2] / xyz[:, 2:]
    return np.round(xy).astype(int)


def fill_closed(mask, pts, value=1):
    """Set mask[y, x] = value for every integer pixel inside or on the boundary of the closed polygon pts ((n, 2) integer x, y; a
    repeated closing vertex is harmless).  Exact integer arithmetic: on-segment by a zero cross product inside the segment's box,
    interior by the even-odd rule on half-open crossings."""
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    H, W = mask.shape
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(H, dtype=np.int64)[:, None]
    inside = np.zeros((H, W), dtype=bool)
    edge = np.zeros((H, W), dtype=bool)
    n = len(pts)
    for i in range(n):
        (ax, ay), (bx, by) = pts[i], pts[(i + 1) % n]
        cross = (bx - ax) * (y - ay) - (by - ay) * (x - ax)
        edge |= (cross == 0) & (x >= min(ax, bx)) & (x <= max(ax, bx)) & (y >= min(ay, by)) & (y <= max(ay, by))
        if ay != by:
            straddle = (ay > y) != (by > y)
            t = (x - ax) * (by - ay) - (y - ay) * (bx - ax)          # x < ax + (y - ay) (bx - ax) / (by - ay), cleared of the division
            left = (t < 0) if by > ay else (t > 0)
            inside ^= straddle & left
    mask[inside | edge] = value
    return mask


def bound_mask(corners_2d, H, W):
    """get_bound_2d_mask (:36-47) from the rounded corners: the union of the six closed quads."""
    mask = np.zeros((H, W), dtype=np.uint8)
    for q in QUADS:
        fill_closed(mask, corners_2d[q + q[:1]], 1)
    return mask


def classes(bmask, body):
    """(class 0, class 1) as boolean images: msk * bound_mask == 1 (:97, :120) and (bound_mask == 1) & (msk != 1) (:130), for a body
    mask that is non-zero where the reference's msk is 1."""
    b = np.asarray(body) != 0
    m = np.asarray(bmask) == 1
    return m & b, m & ~b


def get_rays(H, W, K, R, T):
    """get_rays (:5-18), float64, as per-pixel scalar formulas (3-term dots summed left to right)."""
    K, R, T = np.asarray(K, dtype=np.float64), np.asarray(R, dtype=np.float64), np.asarray(T, dtype=np.float64).reshape(3)
    Ki = np.linalg.inv(K)
    o = -np.array([(R[0, c] * T[0] + R[1, c] * T[1]) + R[2, c] * T[2] for c in range(3)])
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing='xy')
    pc = [(x * Ki[c, 0] + y * Ki[c, 1]) + Ki[c, 2] for c in range(3)]
    q = [pc[c] - T[c] for c in range(3)]
    pw = [(q[0] * R[0, c] + q[1] * R[1, c]) + q[2] * R[2, c] for c in range(3)]
    rays_d = np.stack([pw[c] - o[c] for c in range(3)], axis=2)
    return np.broadcast_to(o, rays_d.shape), rays_d


def get_near_far(bounds, ray_o, ray_d):
    """get_near_far (:50-85) on float64 rays (n, 3); ray_d's exact zeros are replaced in place, as there."""
    b = np.asarray(bounds).astype(np.float64) + np.array([-0.01, 0.01])[:, None]
    ray_d[ray_d == 0.0] = 1e-8
    n = ray_o.shape[0]
    eps = 1e-6
    cnt = np.zeros(n, dtype=np.int64)
    dist = np.zeros((n, 2))
    norm = np.sqrt((ray_d[:, 0] * ray_d[:, 0] + ray_d[:, 1] * ray_d[:, 1]) + ray_d[:, 2] * ray_d[:, 2])
    for k in range(6):                                   # min_x, min_y, min_z, max_x, max_y, max_z
        side, ax = divmod(k, 3)
        t = (b[side, ax] - ray_o[:, ax]) / ray_d[:, ax]
        p = t[:, None] * ray_d + ray_o
        inside = np.ones(n, dtype=bool)
        for c in range(3):
            inside &= (p[:, c] >= b[0, c] - eps) & (p[:, c] <= b[1, c] + eps)
        e = p - ray_o
        r = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) / norm
        first, second = inside & (cnt == 0), inside & (cnt == 1)
        dist[first, 0] = r[first]
        dist[second, 1] = r[second]
        cnt += inside
    mask = cnt == 2
    return np.minimum(dist[mask, 0], dist[mask, 1]), np.maximum(dist[mask, 0], dist[mask, 1]), mask


def round_sizes(missing, ratio):
    """(n_body, n_rand) of a round with `missing` rays to go (:116-117)."""
    n_body = int(missing * ratio)
    return n_body, missing - n_body


def sample_ray_batch(img, body, K, R, T, bounds, nrays, picks, ratio=0.8, max_rounds=32):
    """The split == 'train' loop (:102-170) for one view with the draws injected: picks (rounds, 2, >= nrays) integers, round r taking
    picks[r, 0, :n_body] as its body indices and picks[r, 1, :n_rand] as its background indices.  img (H, W, 3) float32.  Stops after
    max_rounds rounds; rows that stay unfilled are zeros with near 0 and far 1.
    -> dict of rgb, ray_o, ray_d (n, 3) float32, near, far (n,) float32, coord (n, 2) int (y, x), mask_at_box (n,) bool,
       bkgd_msk (n,) int (1 = class 0), n_valid, rounds, bound_mask, corners."""
    H, W = img.shape[:2]
    ray_o, ray_d = get_rays(H, W, K, R, T)
    corners = bound_corners_2d(bounds, K, R, T)
    bmask = bound_mask(corners, H, W)
    c0, c1 = classes(bmask, body)
    coord_body, coord_bkgd = np.argwhere(c0), np.argwhere(c1)
    out = {k: [] for k in ("rgb", "ray_o", "ray_d", "near", "far", "coord", "bkgd_msk")}
    got, rounds = 0, 0
    while got < nrays and rounds < max_rounds:
        n_body, n_rand = round_sizes(nrays - got, ratio)
        coord = np.concatenate([coord_body[np.asarray(picks[rounds][0][:n_body], dtype=np.int64)],
                                coord_bkgd[np.asarray(picks[rounds][1][:n_rand], dtype=np.int64)]], axis=0)
        flag = np.concatenate([np.ones(n_body, dtype=np.int64), np.zeros(n_rand, dtype=np.int64)])
        o_ = ray_o[coord[:, 0], coord[:, 1]]
        d_ = ray_d[coord[:, 0], coord[:, 1]]
        near, far, hit = get_near_far(bounds, o_, d_)
        out["ray_o"].append(o_[hit]), out["ray_d"].append(d_[hit]), out["rgb"].append(img[coord[:, 0], coord[:, 1]][hit])
        out["near"].append(near), out["far"].append(far), out["coord"].append(coord[hit]), out["bkgd_msk"].append(flag[hit])
        got += len(near)
        rounds += 1
    res = {}
    for k, width, dt in (("rgb", 3, np.float32), ("ray_o", 3, np.float32), ("ray_d", 3, np.float32), ("near", 0, np.float32),
                         ("far", 0, np.float32), ("coord", 2, np.int64), ("bkgd_msk", 0, np.int64)):
        full = np.zeros((nrays, width) if width else (nrays,), dtype=dt)
        if k == "far":
            full[:] = 1
        a = np.concatenate(out[k]).astype(dt) if out[k] else full[:0]
        full[:len(a)] = a
        res[k] = full
    res["mask_at_box"] = np.arange(nrays) < got
    res.update(n_valid=got, rounds=rounds, bound_mask=bmask, corners=corners)
    return res


def unpack_bits(words, W):
    """(..., ceil(W / 64)) int64 / uint64 bitmap rows -> (..., W) bool: bit x % 64 of word x // 64."""
    w = np.asarray(words).astype(np.uint64)
    bits = (w[..., :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(*w.shape[:-1], -1)[..., :W].astype(bool)
