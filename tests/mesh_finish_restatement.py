"""Numpy float64 restatement of the mesh-finishing contract (DESIGN.md "Mesh extraction", "Finishing the mesh"): 26-connected
components of the solid side, the component filter and the vertex normals.  Written from the contract, independent of the HIP code
in humanliff_amd/csrc/hl_geometry.hip; the marching cubes it builds on is tests/geometry_restatement.py.
"""
import numpy as np

import geometry_restatement as gr


# Bernoulli volumes for the labelling tests.  Much denser than this, 26-connectivity percolates into one component and a test on
# them shows nothing: these give 142, 2 and 229 components.
BERNOULLI = [((33, 20, 17), 0.12), ((5, 7, 9), 0.3), ((17, 16, 33), 0.06)]


def bernoulli(shape, p):
    return np.random.default_rng(0).random(shape) < p


def solid_of(v, iso):
    return ~(np.asarray(v, dtype=np.float64) > iso)


def label(solid):
    """(labels int32, sizes int64): flood fill with the 26 neighbours, seeds taken in C order, so a component's number is the rank
    of its smallest linear index."""
    solid = np.asarray(solid, dtype=bool)
    nx, ny, nz = solid.shape
    labels = np.zeros(solid.shape, dtype=np.int32)
    offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
    sizes = []
    flat_solid = solid.reshape(-1)
    flat_labels = labels.reshape(-1)
    for seed in np.flatnonzero(flat_solid):
        if flat_labels[seed]:
            continue
        cur = len(sizes) + 1
        flat_labels[seed] = cur
        stack, count = [int(seed)], 0
        while stack:
            i = stack.pop()
            count += 1
            x, y, z = i // (ny * nz), (i // nz) % ny, i % nz
            for dx, dy, dz in offs:
                X, Y, Z = x + dx, y + dy, z + dz
                if 0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz:
                    j = (X * ny + Y) * nz + Z
                    if flat_solid[j] and not flat_labels[j]:
                        flat_labels[j] = cur
                        stack.append(j)
        sizes.append(count)
    return labels, np.asarray(sizes, dtype=np.int64)


def label_volume(v, iso):
    return label(solid_of(v, iso))


def select(sizes, keep):
    """Kept labels (1-based, ascending): "largest", an int k, or ("min_voxels", m); ties in size go to the lower label."""
    n = len(sizes)
    if isinstance(keep, tuple):
        assert keep[0] == "min_voxels"
        return np.asarray([l + 1 for l in range(n) if sizes[l] >= keep[1]], dtype=np.int64)
    k = 1 if keep == "largest" else int(keep)
    order = sorted(range(n), key=lambda l: (-int(sizes[l]), l))
    return np.asarray(sorted(l + 1 for l in order[:k]), dtype=np.int64)


def filter_volume(v, iso, labels, kept):
    v = np.asarray(v, dtype=np.float64)
    dropped = (labels > 0) & ~np.isin(labels, kept)
    with np.errstate(invalid="ignore"):
        w = iso + np.abs(v - iso)
        w = np.where(w > iso, w, np.nextafter(np.float64(iso), np.inf))
    out = v.copy()
    out[dropped] = w[dropped]
    return out


def keep_components(v, iso, keep):
    labels, sizes = label_volume(v, iso)
    kept = select(sizes, keep)
    return filter_volume(v, iso, labels, kept), kept


def triangle_cells(v, iso):
    """Lower corner (T,3) of the cell of every triangle of gr.marching_cubes(v, iso), in its triangle order (by cube, C order)."""
    v = np.asarray(v, dtype=np.float64)
    nx, ny, nz = v.shape
    above = v > iso
    cfg = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = gr.CORNERS[c]
        cfg |= above[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ntri = np.array([len(t) for t in gr.case_table()])
    cube = np.argwhere(ntri[cfg] > 0)
    return np.repeat(cube, ntri[cfg[cube[:, 0], cube[:, 1], cube[:, 2]]], axis=0)


def expected_subset(v, iso, labels, kept, cells):
    """Which triangles of mc(v) the filtered volume must keep: those whose cell has a kept solid corner, or no solid corner of a
    dropped component (a cell never holds solid corners of two components: its corners are pairwise 26-adjacent)."""
    keep_tri = np.zeros(len(cells), dtype=bool)
    has_dropped = np.zeros(len(cells), dtype=bool)
    for c in range(8):
        p = cells + gr.CORNERS[c]
        l = labels[p[:, 0], p[:, 1], p[:, 2]]
        k = np.isin(l, kept)
        keep_tri |= (l > 0) & k
        has_dropped |= (l > 0) & ~k
    assert not (keep_tri & has_dropped).any()
    return keep_tri | ~has_dropped


def check_subset(full, filtered, expect):
    """mc(keep(vol)) against mc(vol): exactly the expected triangles, in order, and bit-equal vertices after re-indexing."""
    (v0, t0), (v1, t1) = full, filtered
    sub = t0[expect]
    assert len(sub) == len(t1), (len(sub), len(t1))
    used = np.unique(sub)
    assert len(used) == len(v1)                            # no vertex of the filtered mesh is left unused or new
    remap = np.full(len(v0) + 1, -1, dtype=np.int64)
    remap[used] = np.arange(len(used))                     # (vertices are ordered by edge key on both sides: a monotone map)
    assert np.array_equal(remap[sub], t1)
    assert np.array_equal(v0[used], v1)


def gradient(v):
    """(3, nx, ny, nz): central differences, one-sided at the faces, 0 along an axis of one voxel."""
    v = np.asarray(v, dtype=np.float64)
    g = np.zeros((3,) + v.shape)
    for a in range(3):
        n = v.shape[a]
        if n < 2:
            continue
        sl = lambda s: tuple(s if k == a else slice(None) for k in range(3))  # noqa: E731
        g[a][sl(slice(1, n - 1))] = (v[sl(slice(2, n))] - v[sl(slice(0, n - 2))]) * 0.5
        g[a][sl(slice(0, 1))] = v[sl(slice(1, 2))] - v[sl(slice(0, 1))]
        g[a][sl(slice(n - 1, n))] = v[sl(slice(n - 1, n))] - v[sl(slice(n - 2, n - 1))]
    return g


def vertex_normals(v, iso, extent=None):
    """Normals (V,3) of gr.marching_cubes(v, iso)'s vertices, in its order (edge keys)."""
    v = np.asarray(v, dtype=np.float64)
    nx, ny, nz = v.shape
    ext = np.ones(3) if extent is None else np.asarray(extent, dtype=np.float64)
    above = v > iso
    g = gradient(v)
    keys, nrm = [], []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a] = slice(0, v.shape[a] - 1)
        hi[a] = slice(1, None)
        crossing = above[tuple(lo)] != above[tuple(hi)]
        p = np.argwhere(crossing)
        fa = v[tuple(lo)][crossing]
        fb = v[tuple(hi)][crossing]
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (iso - fa) / (fb - fa)
        q = p.copy()
        q[:, a] += 1
        ga = g[:, p[:, 0], p[:, 1], p[:, 2]].T
        gb = g[:, q[:, 0], q[:, 1], q[:, 2]].T
        with np.errstate(invalid="ignore"):
            n = ((1.0 - t)[:, None] * ga + t[:, None] * gb) / ext[None, :]
        keys.append(((p[:, 0] * ny + p[:, 1]) * nz + p[:, 2]) * 3 + a)
        nrm.append(n)
    keys = np.concatenate(keys)
    n = np.concatenate(nrm)[np.argsort(keys, kind="stable")]
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        ok = (length > 0) & (length < np.inf)
        return np.where(ok[:, None], n / np.where(ok, length, 1.0)[:, None], 0.0)
