"""GPU: hl_view_ingest (csrc/hl_view_ingest.hip through humanliff_amd.view_ingest) against the restatement of its contract
(tests/view_ingest_restatement.py) on the seeded cases of tests/view_ingest_cases.py."""
import numpy as np
import pytest
import torch

from tests import view_ingest_cases as vc

pytestmark = pytest.mark.gpu
NAMES = list(vc.CASES)


def own_bound(src, H, W):
    """The rule of tests/view_ingest_cases.py for a shape outside the committed cases: twice the gap between the float32 and the float64
    restatement of that shape."""
    from tests import view_ingest_restatement as vr
    return 2 * float(np.abs(vr.resize_area_f32(src, H, W).astype(np.float64) - vr.resize_area_f64(src, H, W)).max())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def results(dev):
    """name -> (image (3, H, W, 3) float32, body (3, H, W) uint8) host arrays of one V = 3 call per case (computed once, read only)."""
    from humanliff_amd.view_ingest import ingest_views
    out = {}
    for name in NAMES:
        img, msk = vc.case(name)
        image, body = ingest_views(torch.from_numpy(img.copy()).to(dev), torch.from_numpy(msk.copy()).to(dev), *vc.target_size(name))
        assert image.dtype == torch.float32 and body.dtype == torch.uint8
        assert tuple(image.shape) == (3, *vc.target_size(name), 3) and tuple(body.shape) == (3, *vc.target_size(name))
        out[name] = (image.cpu().numpy(), body.cpu().numpy())
    return out


@pytest.mark.parametrize("name", NAMES)
def test_body_is_the_nearest_rule_bit_for_bit(results, name):
    assert np.array_equal(results[name][1], vc.reference(name)["body"])


@pytest.mark.parametrize("name", NAMES)
def test_image_within_the_bound_of_the_float64_restatement(results, name):
    ref = vc.reference(name)
    got = results[name][0]
    err = float(np.abs(got.astype(np.float64) - ref["f64"]).max())
    same = float((got == ref["f32"]).mean())
    print(f"{name}: max |device - float64 restatement| {err:.4e} (bound {vc.DEVICE_BOUND:.4e}); "
          f"{100 * same:.1f} % of the values equal the float32 restatement bit for bit")
    assert err <= vc.DEVICE_BOUND


@pytest.mark.parametrize("name", NAMES)
def test_fully_masked_windows_are_exact_zeros(results, name):
    dark = vc.reference(name)["dark"]
    got = results[name][0]
    assert dark.any() and not got[dark].any()
    assert (got[~dark].max(axis=-1) > 0).any()


def test_scale_one_is_the_masked_source_bit_for_bit(results):
    image, body = results["copy"]
    assert np.array_equal(image, vc.reference("copy")["source"])
    assert np.array_equal(body, (vc.case("copy")[1] != 0).astype(np.uint8))


def test_one_axis_at_scale_one(dev):
    """37 x 53 -> 37 x 26 and -> 18 x 53: the general kernel with a one-tap table on one axis."""
    from humanliff_amd.view_ingest import ingest_views
    from tests import view_ingest_restatement as vr
    img, msk = vc.case("ragged")
    src = vc.reference("ragged")["source"]
    for H, W in ((37, 26), (18, 53)):
        image, body = ingest_views(torch.from_numpy(img.copy()).to(dev), torch.from_numpy(msk.copy()).to(dev), H, W)
        err = float(np.abs(image.cpu().numpy().astype(np.float64) - vr.resize_area_f64(src, H, W)).max())
        bound = own_bound(src, H, W)
        print(f"37 x 53 -> {H} x {W}: max error {err:.4e} (bound {bound:.4e})")
        assert err <= bound
        assert np.array_equal(body.cpu().numpy(), vr.resize_nearest(msk, H, W))


def test_more_than_one_tile_and_unaligned_rows(dev):
    """1 x (5, 1031) -> (2, 515): three 256-pixel tiles in a row, source rows that start at odd addresses; V = 1 of odd size so the last 16-byte
    chunk crosses the end of the arrays."""
    from humanliff_amd.view_ingest import ingest_views
    from tests import view_ingest_restatement as vr
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (1, 5, 1031, 3), dtype=np.uint8)
    msk = (rng.random((1, 5, 1031)) < 0.7).astype(np.uint8) * 255
    image, body = ingest_views(torch.from_numpy(img).to(dev), torch.from_numpy(msk).to(dev), 2, 515)
    src = vr.masked_source(img, msk)
    got = image.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - vr.resize_area_f64(src, 2, 515)).max())
    bound = own_bound(src, 2, 515)
    print(f"5 x 1031 -> 2 x 515: max error {err:.4e} (bound {bound:.4e})")
    assert err <= bound
    assert np.array_equal(body.cpu().numpy(), vr.resize_nearest(msk, 2, 515))


@pytest.mark.parametrize("name", NAMES)
def test_runs_repeat_and_views_do_not_depend_on_the_batch(dev, results, name):
    from humanliff_amd.view_ingest import ingest_views
    img, msk = vc.case(name)
    H, W = vc.target_size(name)
    d_img, d_msk = torch.from_numpy(img.copy()).to(dev), torch.from_numpy(msk.copy()).to(dev)
    image, body = ingest_views(d_img, d_msk, H, W)
    assert np.array_equal(image.cpu().numpy(), results[name][0]) and np.array_equal(body.cpu().numpy(), results[name][1])
    for v in range(vc.VIEWS):                                         # (a slice of the batch is copied to an aligned tensor by the wrapper)
        one_image, one_body = ingest_views(d_img[v:v + 1], d_msk[v:v + 1], H, W)
        assert torch.equal(one_image[0], image[v]) and torch.equal(one_body[0], body[v]), (name, v)


def test_enlarging_raises(dev):
    from humanliff_amd.view_ingest import ingest_views
    img, msk = vc.case("tiny")
    d_img, d_msk = torch.from_numpy(img.copy()).to(dev), torch.from_numpy(msk.copy()).to(dev)
    with pytest.raises(ValueError):
        ingest_views(d_img, d_msk, 8, 9)
    with pytest.raises(ValueError):
        ingest_views(d_img, d_msk, 7, 10)
    with pytest.raises(TypeError):
        ingest_views(d_img.float(), d_msk, 3, 4)
