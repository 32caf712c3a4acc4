"""GPU: hl_view_ingest_layers (csrc/hl_view_ingest.hip through humanliff_amd.view_ingest.ingest_layered_views) against the restatement of
its contract (tests/tightcap_restatement.py, pinned to the reference by tests/golden/tightcap_layers.npz) on the seeded cases of
tests/tightcap_cases.py."""
import os

import numpy as np
import pytest
import torch

from tests import tightcap_cases as tc
from tests import tightcap_restatement as tr

pytestmark = pytest.mark.gpu
NAMES = list(tc.REDUCTIONS)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tightcap_layers.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def upload(img, planes, dev, only=None):
    """Device copies; `only`: the names of the planes to supply (the others are None)."""
    d_planes = {n: (torch.from_numpy(p.copy()).to(dev) if only is None or n in only else None) for n, p in planes.items()}
    return torch.from_numpy(img.copy()).to(dev), d_planes


@pytest.fixture(scope="module")
def results(dev):
    """name -> (image, body) host arrays of one call per case, every plane supplied (computed once, read only)."""
    from humanliff_amd.view_ingest import ingest_layered_views
    out = {}
    for name in NAMES + ["copy"]:
        img, planes, layers, H, W = tc.case(name)
        d_img, d_planes = upload(img, planes, dev)
        image, body = ingest_layered_views(d_img, d_planes, layers.tolist(), H, W)
        assert image.dtype == torch.float32 and body.dtype == torch.uint8
        assert tuple(image.shape) == (len(layers), H, W, 3) and tuple(body.shape) == (len(layers), H, W)
        out[name] = (image.cpu().numpy(), body.cpu().numpy())
    return out


def test_scale_one_is_the_composed_source_bit_for_bit(results):
    """5 views of 9 x 15 with the layers mixed: 675 pixels, so groups of four straddle views and the last three go bytewise."""
    img, planes, layers, H, W = tc.case("copy")
    assert (len(layers) * H * W) % 4 != 0 and (H * W) % 4 != 0 and set(layers.tolist()) == {0, 1, 2, 3}
    ref = tc.reference("copy")
    image, body = results["copy"]
    assert np.array_equal(image, ref["source"]) and np.array_equal(body, ref["mask"])
    assert 0 < body.sum() < body.size and (image == tr.SKIN).all(axis=-1).any()


def test_scale_one_equals_the_reference(dev):
    """The golden's own sources: every layer of its two views in one batch equals what TightCapDatasetBatch.__getitem__ returned."""
    from humanliff_amd.view_ingest import ingest_layered_views
    g = np.load(GOLDEN)
    views, layers = g["views"], g["layers"]
    planes = {n: g["plane_" + n][views] for n in tr.PLANES}
    d_img, d_planes = upload(g["img_u8"][views], planes, dev)
    image, body = ingest_layered_views(d_img, d_planes, layers.tolist(), 24, 28)
    assert np.array_equal(image.cpu().numpy().transpose(0, 3, 1, 2), g["img_all"])
    assert np.array_equal(body.cpu().numpy().astype(np.float64), g["msk_all"])


@pytest.mark.parametrize("name", NAMES)
def test_reduction_within_the_bound_of_the_float64_restatement(results, name):
    ref = tc.reference(name)
    got, body = results[name]
    bound = tc.own_bound(ref)
    err = float(np.abs(got.astype(np.float64) - ref["f64"]).max())
    same = float((got == ref["f32"]).mean())
    print(f"{name}: max |device - float64 restatement| {err:.4e} (bound {bound:.4e} = twice the float32 restatement's gap); "
          f"{100 * same:.1f} % of the values equal the float32 restatement bit for bit")
    assert bound > 0.0
    assert err <= bound
    assert np.array_equal(body, ref["body"])                                             # the nearest rule of the derived mask
    assert 0 < body.sum() < body.size


@pytest.mark.parametrize("name", NAMES + ["copy"])
def test_unread_planes_are_never_looked_at(dev, results, name):
    """Every (view, plane) the view's layer does not name is filled with 0xAA: the outputs do not change.  Nor do they when the planes no
    view of the batch names are not supplied at all."""
    from humanliff_amd.view_ingest import LAYER_PLANES, ingest_layered_views, planes_read
    img, planes, layers, H, W = tc.case(name)
    poisoned = {n: p.copy() for n, p in planes.items()}
    for v, layer in enumerate(layers):
        for n in tr.PLANES:
            if n not in LAYER_PLANES[layer]:
                poisoned[n][v] = 0xAA
    d_img, d_planes = upload(img, poisoned, dev)
    image, body = ingest_layered_views(d_img, d_planes, layers.tolist(), H, W)
    assert np.array_equal(image.cpu().numpy(), results[name][0]) and np.array_equal(body.cpu().numpy(), results[name][1])
    for sub in ([3], [2, 3], [1, 2]):                                                     # batches that read one, three and four planes
        keep = [v for v, layer in enumerate(layers) if layer in sub]
        if not keep:
            continue
        sel = {n: p[keep] for n, p in poisoned.items()}
        d_img, d_all = upload(img[keep], sel, dev)
        _, d_some = upload(img[keep], sel, dev, only=planes_read(layers[keep].tolist()))
        assert any(p is None for p in d_some.values())
        a = ingest_layered_views(d_img, d_all, layers[keep].tolist(), H, W)
        b = ingest_layered_views(d_img, tuple(d_some[n] for n in tr.PLANES), layers[keep].tolist(), H, W)    # (the 5-tuple form)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert np.array_equal(a[0].cpu().numpy(), results[name][0][keep]) and np.array_equal(a[1].cpu().numpy(), results[name][1][keep])


@pytest.mark.parametrize("name", ["int2", "ragged", "tiles", "copy"])
def test_layer_three_is_the_plain_ingest_bit_for_bit(dev, name):
    from humanliff_amd.view_ingest import ingest_layered_views, ingest_views
    img, planes, layers, H, W = tc.case(name)
    d_img, d_planes = upload(img, planes, dev, only=("full",))
    image, body = ingest_layered_views(d_img, d_planes, [3] * len(layers), H, W)
    want_image, want_body = ingest_views(d_img, d_planes["full"], H, W)
    assert torch.equal(image, want_image) and torch.equal(body, want_body)


@pytest.mark.parametrize("name", NAMES + ["copy"])
def test_runs_repeat_and_views_do_not_depend_on_the_batch(dev, results, name):
    from humanliff_amd.view_ingest import ingest_layered_views
    img, planes, layers, H, W = tc.case(name)
    d_img, d_planes = upload(img, planes, dev)
    image, body = ingest_layered_views(d_img, d_planes, layers.tolist(), H, W)
    assert np.array_equal(image.cpu().numpy(), results[name][0]) and np.array_equal(body.cpu().numpy(), results[name][1])
    for v in range(len(layers)):                                      # (a slice of the batch is copied to an aligned tensor by the wrapper)
        one_image, one_body = ingest_layered_views(d_img[v:v + 1], {n: p[v:v + 1] for n, p in d_planes.items()}, [int(layers[v])], H, W)
        assert torch.equal(one_image[0], image[v]) and torch.equal(one_body[0], body[v]), (name, v)


def test_bad_input_raises(dev):
    from humanliff_amd.view_ingest import ingest_layered_views
    img, planes, layers, H, W = tc.case("tiny")
    d_img, d_planes = upload(img, planes, dev)
    L = layers.tolist()
    with pytest.raises(ValueError):
        ingest_layered_views(d_img, d_planes, L, 8, 9)                                   # enlarging
    with pytest.raises(ValueError):
        ingest_layered_views(d_img, d_planes, L, 7, 10)
    with pytest.raises(TypeError):
        ingest_layered_views(d_img.float(), d_planes, L, 3, 4)
    with pytest.raises(TypeError):
        ingest_layered_views(d_img, dict(d_planes, top=d_planes["top"].int()), L, 3, 4)
    with pytest.raises(ValueError):
        ingest_layered_views(d_img, dict(d_planes, shoes=d_planes["shoes"][:, :-1]), L, 3, 4)
    with pytest.raises(ValueError):
        ingest_layered_views(d_img, d_planes, [0, 1, 2, 4], 3, 4)                        # a layer outside 0 .. 3
    with pytest.raises(ValueError):
        ingest_layered_views(d_img, d_planes, [0, 1, -1, 3], 3, 4)
    with pytest.raises(ValueError):
        ingest_layered_views(d_img, d_planes, [0, 1, 2], 3, 4)                           # a layer per view
    with pytest.raises(ValueError, match="bottom"):
        ingest_layered_views(d_img, dict(d_planes, bottom=None), L, 3, 4)                # layer 0 reads the bottom
    with pytest.raises(ValueError):
        ingest_layered_views(d_img, (d_planes["full"],), L, 3, 4)
    with pytest.raises(ValueError):
        ingest_layered_views(d_img, dict(d_planes, hat=d_planes["top"]), L, 3, 4)
    with pytest.raises(RuntimeError):
        ingest_layered_views(d_img.cpu(), d_planes, L, 3, 4)
