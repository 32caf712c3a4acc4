"""Host-side (no GPU) checks of the product package: state_dict layout, schedules, factories,
the C-ABI library (loads, exports every declared symbol), loud failure without a GPU."""
import ast
import os
import re

import numpy as np
import pytest
import torch

from tests.golden_util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(over):
    from humanliff_amd.improved_diffusion.script_util import model_and_diffusion_defaults
    a = model_and_diffusion_defaults()
    a.update(dict(in_channels=27, out_channels=27, class_cond=True, learn_sigma=False, num_heads=4, rescale_timesteps=False))
    a.update(over)
    return a


@pytest.mark.parametrize("name", ["tiny32", "mid64", "deep256"])
def test_unet_state_dict_layout_equals_reference(name):
    """Keys, order and shapes of UNetModel.state_dict() == the reference's (stored in the fixture)."""
    from humanliff_amd.improved_diffusion.script_util import create_model_and_diffusion
    g = np.load(os.path.join(GOLDEN, f"unet_{name}.npz"))
    over = dict(image_size=int(g["arg_image_size"]), num_channels=int(g["arg_num_channels"]),
                num_res_blocks=int(g["arg_num_res_blocks"]), attention_resolutions=str(g["arg_attention_resolutions"]))
    model, diffusion = create_model_and_diffusion(**_args(over))
    mine = [(k, list(v.shape)) for k, v in model.state_dict().items()]
    ref = [(str(k), ast.literal_eval(str(s))) for k, s in zip(g["keys"], g["shapes"])]
    assert mine == ref
    assert sum(p.numel() for p in model.parameters()) == int(g["n_params"])
    # zero_module'd tensors start at zero like the reference (unet.py:170, 240, 470, 486)
    sd = model.state_dict()
    for k in sd:
        if re.search(r"out_layers\.3\.|proj_out\.|^out\.2\.|input_blocks_proj_cond", k):
            assert float(sd[k].abs().max()) == 0.0, k


def test_production_config_counts():
    from humanliff_amd.improved_diffusion.script_util import create_model_and_diffusion
    m, d = create_model_and_diffusion(**_args(dict(image_size=256, num_channels=192, num_res_blocks=3,
                                                    attention_resolutions="32,16,8", timestep_respacing="250")))
    assert sum(p.numel() for p in m.parameters()) == 497173083
    assert len(m.state_dict()) == 953
    assert d.num_timesteps == 250 and d.timestep_map[:5] == [0, 4, 8, 12, 16] and d.timestep_map[-1] == 999


@pytest.mark.parametrize("tag,spec", [("full", ""), ("r250", "250"), ("ddim50", "ddim50"), ("ddim10", "ddim10"),
                                      ("mix", "10,15,20")])
def test_spaced_diffusion_tables_equal_reference(tag, spec):
    from humanliff_amd.improved_diffusion.script_util import create_gaussian_diffusion
    g = np.load(os.path.join(GOLDEN, "diffusion_steps.npz"))
    d = create_gaussian_diffusion(steps=1000, timestep_respacing=spec)
    assert d.timestep_map == list(g[f"{tag}_map"])
    assert np.array_equal(d.betas, g[f"{tag}_betas"])
    assert np.array_equal(d.posterior_log_variance_clipped, g[f"{tag}_post_logvar"])
    assert np.array_equal(d.posterior_mean_coef1, g[f"{tag}_coef1"])
    assert np.array_equal(d.posterior_mean_coef2, g[f"{tag}_coef2"])
    assert np.array_equal(d.sqrt_recip_alphas_cumprod, g[f"{tag}_sqrt_recip"])
    assert np.array_equal(d.sqrt_recipm1_alphas_cumprod, g[f"{tag}_sqrt_recipm1"])


def test_schedule_errors_match_reference_types():
    from humanliff_amd.improved_diffusion import gaussian_diffusion as gd
    from humanliff_amd.improved_diffusion.respace import space_timesteps
    from humanliff_amd.improved_diffusion.script_util import create_model
    g = np.load(os.path.join(GOLDEN, "diffusion_steps.npz"))
    assert np.array_equal(gd.get_named_beta_schedule("cosine", 50), g["cosine50_betas"])
    with pytest.raises(NotImplementedError):
        gd.get_named_beta_schedule("quadratic", 10)
    with pytest.raises(ValueError):
        space_timesteps(1000, "ddim999")
    with pytest.raises(ValueError):
        space_timesteps(10, "20")
    with pytest.raises(ValueError):       # script_util.py:124
        create_model(100, 27, 32, 27, 1, False, True, False, "16,8", 4, -1, True, "controlnet", False, 0.0)


def test_library_exports_every_declared_symbol():
    from humanliff_amd import _lib
    from humanliff_amd.build import build
    build()
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "humanliff_hip.h")).read()
    declared = set(re.findall(r"\b(hl_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"hl_status"}
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/humanliff_hip.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert L.hl_version() >= 100
    assert L.hl_render_mlp_packed_bytes() == (17 * 4096 + 1024) * 4 + 132 * 1024 + 3 * 132 * 1024 + 2 * 132 * 1024      # fp32 image + the 132 fp16 fragments of k_march16 + the three bf16 planes (bf16x3) + the two fp16 planes (fp16x2)
    assert L.hl_planes_packed_bytes(256, 256) == 9 * 256 * 256 * 16


_CONV_LAYERS = [   # (N, H, W, Cin, Cout, ks, stride, upsample)
    (2, 8, 8, 384, 1152, 1, 1, 0), (4, 8, 8, 768, 768, 3, 1, 0), (2, 32, 32, 192, 192, 3, 1, 0), (2, 16, 16, 64, 64, 3, 2, 0),
    (2, 8, 8, 64, 64, 3, 1, 1), (1, 12, 20, 96, 27, 3, 1, 0), (3, 5, 7, 16, 80, 1, 1, 0),
    (4, 8, 8, 256, 192, 3, 1, 1), (4, 16, 16, 256, 192, 3, 1, 0), (2, 32, 32, 384, 384, 3, 1, 0), (1, 16, 16, 384, 1152, 1, 1, 0)]   # a GroupNorm in front changes the kernel family


@pytest.mark.parametrize("layer", _CONV_LAYERS)
def test_conv_scratch_queries(layer):
    """The scratch queries of the single-op convolutions are host arithmetic: every region is rounded to 256 bytes, the GroupNorm input
    adds exactly its own size, and the entry points with a prefix never ask for less than the plain call."""
    from humanliff_amd import _lib
    from humanliff_amd.build import build
    build()
    L = _lib.lib()
    N, H, W, Cin, Cout, ks, stride, ups = layer
    Hv, Wv = (2 * H, 2 * W) if ups else (H, W)
    Ho, Wo = (Hv + 2 * (ks // 2) - ks) // stride + 1, (Wv + 2 * (ks // 2) - ks) // stride + 1
    act = (N * H * W * Cin * 4 + 255) // 256 * 256
    for mode in (_lib.HL_CONV_FP32, _lib.HL_CONV_FP32_DIRECT, _lib.HL_CONV_BF16, _lib.HL_CONV_FP16):
        plain = L.hl_conv2d_scratch_bytes(mode, N, H, W, Cin, Cout, ks, stride, ups, 0)
        with_gn = L.hl_conv2d_scratch_bytes(mode, N, H, W, Cin, Cout, ks, stride, ups, 1)
        assert plain >= (Cout + 63) // 64 * 64 * Cin * ks * ks * 4 and plain % 256 == 0
        assert with_gn == (0 if ups else plain + act)            # (a GroupNorm in front of an upsample: no call accepts it, tests/test_conv_fwd_cpu.py)
        for gn in (0, 1):
            fused = L.hl_conv2d_gn_scratch_bytes(mode, N, H, W, Cin, Cout, ks, stride, ups, gn)
            assert fused == 0 if (gn and ups) else (fused % 256 == 0 and fused >= (with_gn if gn else plain))
        # the backward-data of this layer: d output (N,Ho,Wo,Cout) -> d input (N,H,W,Cin), a convolution Cout -> Cin on the gradient's grid
        Cy = (Cout + 15) // 16 * 16
        back = L.hl_conv2d_bwd_data_scratch_bytes(mode, N, Ho, Wo, Cy, Cout, Cin, ks, stride, ups, Cin)
        # the zero-stuffed / upsampled gradient in front of the room of the convolution it runs: Cy -> Cin on the gradient's grid, flipped weights,
        # no GroupNorm.  Flipped weights have no fp16x2 form and a forward layer keeps room for the slabs of either plan (with / without
        # GroupNorm), so this is not "the plain query plus a prefix": between the packed fp32 weights and the forward query of that geometry
        s = 2 if stride == 2 else 1
        front = (N * 4 * Ho * Wo * Cy * 4 + 255) // 256 * 256 if stride == 2 else (N * Ho * Wo * Cin * 4 + 255) // 256 * 256 if ups else 0
        w32 = (Cin + 63) // 64 * 64 * Cy * ks * ks * 4
        assert back % 256 == 0 and back >= front + w32
        if mode != _lib.HL_CONV_FP32:
            assert back <= front + L.hl_conv2d_scratch_bytes(mode, N, s * Ho, s * Wo, Cy, Cin, ks, 1, 0, 0)
    # hl_conv2d_nhwc is the query at HL_CONV_FP32_DIRECT: its refusal (the size check comes before any use of a pointer) names both numbers
    rc = L.hl_conv2d_nhwc(None, N, H, W, Cin, None, None, Cout, ks, stride, ups, None, None, 0, None, None, None, 0, None)
    msg = L.hl_last_error().decode()
    want = L.hl_conv2d_scratch_bytes(_lib.HL_CONV_FP32_DIRECT, N, H, W, Cin, Cout, ks, stride, ups, 0)
    assert rc == -1 and "hl_conv2d_scratch_bytes" in msg and re.search(r"\(0 bytes, hl_conv2d_scratch_bytes says (\d+)\)", msg).group(1) == str(want)


def test_conv_scratch_queries_give_zero_for_arguments_no_call_accepts():
    from humanliff_amd import _lib
    from humanliff_amd.build import build
    build()
    L = _lib.lib()
    good = dict(mode=0, N=2, H=8, W=8, Cin=64, Cout=64, ks=3, stride=1, ups=0)
    assert L.hl_conv2d_scratch_bytes(*good.values(), 0) > 0
    for bad in (dict(stride=0), dict(stride=3), dict(N=0), dict(H=0), dict(W=-1), dict(Cin=24), dict(Cin=0), dict(Cout=0), dict(ks=2), dict(mode=99)):
        a = list({**good, **bad}.values())
        assert L.hl_conv2d_scratch_bytes(*a, 0) == 0 and L.hl_conv2d_gn_scratch_bytes(*a, 1) == 0, bad
        mode, N, H, W, Cin, Cout, ks, stride, ups = a
        assert L.hl_conv2d_bwd_data_scratch_bytes(mode, N, H, W, Cin, Cin, Cout, ks, stride, ups, Cout) == 0, bad


def test_training_scratch_queries():
    from humanliff_amd import _lib
    from humanliff_amd.build import build
    build()
    L = _lib.lib()
    for N in (1, 3):
        assert L.hl_groupnorm_scratch_bytes(N) == N * 8192 * 4      # 128 chunks x 32 groups x (sum, sum of squares) per image
        assert L.hl_groupnorm_train_backward_scratch_bytes(N, 256, 64) == N * 64 * 5 * 4 + L.hl_gn_backward_scratch_bytes(N, 256, 64)
        assert L.hl_triplane_agg_backward_scratch_bytes(N, 16, 16, 24) == N * 3 * 32 * 24 * 4


def test_render_size_queries():
    """The renderer's size queries are host arithmetic with closed forms: the tile-major workspace of a render call (rays rounded up to
    tiles of 32, float4 records of both passes + the new depths, + 256), the canonical schedule's two float4 buffers behind it (+ 512),
    the scratch of the backward kernels and the backward pack.  No byte of these layouts moves unnoticed."""
    import ctypes
    from humanliff_amd import _lib
    from humanliff_amd.build import build
    build()
    L = _lib.lib()
    ceil = lambda a, b: -(-a // b)  # noqa: E731
    up256 = lambda b: ceil(b, 256) * 256  # noqa: E731
    for R, N, Ni in [(1, 32, 32), (33, 32, 32), (257, 64, 64), (2048, 128, 128), (262144, 128, 128), (777, 3, 3)]:
        T32 = ceil(R, 32) * 32
        ws = T32 * ((N + Ni) * 4 + Ni) * 4 + 256
        assert L.hl_render_workspace_bytes(R, N, Ni) == ws
        assert L.hl_render_canonical_workspace_bytes(R, N, Ni) == ws + T32 * max(N, Ni) * 32 + 512
        assert L.hl_render_composite_backward_scratch_bytes(R, N, Ni) == T32 * (N + Ni) * 8
        pg = up256(T32 // 32 * 27 * 4)
        assert L.hl_render_plane_grads_scratch_bytes(R) == pg
        assert L.hl_render_plane_grads_points_scratch_bytes(R, N, Ni) == pg + R * (ceil(N, 64) + ceil(Ni, 64)) * 24 + 256
        P = T32 * (N + Ni)
        per = max(1024, ceil(ceil(P, 256), 32) * 32)
        assert L.hl_render_weight_grads_scratch_bytes(P) == ceil(P, per) * 66884 * 4      # 66 884 = the MLP's parameter count
    assert L.hl_render_workspace_bytes(0, 32, 32) == 256 and L.hl_render_workspace_bytes(64, 32, 0) == 256
    assert L.hl_render_canonical_workspace_bytes(0, 32, 32) == 256 and L.hl_render_canonical_workspace_bytes(64, 32, 0) == 140032
    assert L.hl_render_weight_grads_scratch_bytes(0) == 0
    assert L.hl_render_mlp_bwd_packed_bytes() == 524352
    act_rows, del_rows = ctypes.c_int(0), ctypes.c_int(0)
    L.hl_render_train_rows(ctypes.byref(act_rows), ctypes.byref(del_rows))
    assert (act_rows.value, del_rows.value) == (630, 634)


def test_no_cpu_fallback():
    """CPU tensors must fail loudly, never silently route to PyTorch."""
    from humanliff_amd.NeRF import Renderer
    from humanliff_amd.improved_diffusion.script_util import create_model_and_diffusion
    m, d = create_model_and_diffusion(**_args(dict(image_size=32, num_channels=32, num_res_blocks=1)))
    x = torch.zeros(1, 27, 32, 32)
    with pytest.raises(RuntimeError):
        m(x, torch.tensor([3]), x, y=torch.tensor([0]))
    with pytest.raises(RuntimeError):
        d.p_sample(lambda *a, **k: x, x, x, torch.tensor([3]))
    r = Renderer(use_canonical_space=False, triplane_ch=27, test=True)
    with pytest.raises((RuntimeError, AssertionError)):
        r.render({"world_bounds": torch.zeros(1, 2, 3)}, None, None, torch.zeros(1, 4, 3), torch.ones(1, 4, 3),
                 torch.zeros(1, 4), torch.ones(1, 4), torch.zeros(1, 3, 9, 8, 8), 0, False, n_samples=4)


def test_product_never_imports_oracle():
    for base, _, files in os.walk(os.path.join(ROOT, "humanliff_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(base, f)).read()
                assert "oracle" not in src, f"{f} mentions the oracle"


def test_recon_twin_mirrors_reference_names():
    """recon_NeRF/lib/renderer.py:13-29, 244 and run_nerf_batch.py:29: constructor / render argument names and the tri_planes Parameter."""
    import inspect
    from humanliff_amd.recon_NeRF import Renderer, render
    r = Renderer(use_canonical_space=False, num_instances=2, triplane_dim=16, triplane_ch=27, test=False)
    assert list(inspect.signature(Renderer.__init__).parameters)[1:] == ["use_canonical_space", "num_instances", "triplane_dim", "triplane_ch", "test"]
    assert tuple(r.tri_planes.shape) == (2, 4, 3, 9, 16, 16) and r.tri_planes.requires_grad
    assert list(inspect.signature(r.render).parameters)[:9] == ["tp_input", "world_pts", "z_vals", "rays_o", "rays_d", "near", "far",
                                                                 "n_importance", "white_bkgd"]
    assert list(inspect.signature(render).parameters) == ["chunk", "rays_o", "rays_d", "near", "far", "tp_input", "renderer", "n_samples",
                                                          "perturb", "n_importance", "white_bkgd"]
    keys = set(r.state_dict().keys())
    assert {"tri_planes", "pts_linears.0.weight", "alpha_linear.bias", "views_linear.weight", "rgb_linear.bias"} <= keys


def test_spaced_diffusion_wrapper_keeps_temporary_callables_alive_and_releases_models():
    """SpacedDiffusion._wrap_model: the wrapper handed to a loop holds its model strongly (a lambda / functools.partial / bound method passed
    inline must survive the loop: round-3 advisor finding), the per-model cache holds it weakly (deleting a model frees it) and the device
    tensor of the timestep map is built once per model and (device, dtype), not per call like the reference (respace.py:117-122)."""
    import functools
    import gc
    import weakref
    from humanliff_amd.improved_diffusion.script_util import create_gaussian_diffusion
    d = create_gaussian_diffusion(steps=1000, timestep_respacing="ddim10")

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x, t, x_cond, **kw):
            return x * 0 + t.float().reshape(-1, 1)

    m = M()
    for make in (lambda: (lambda x, t, xc, **kw: m(x, t, xc, **kw)), lambda: functools.partial(m.forward), lambda: m.forward):
        w = d._wrap_model(make())                 # the only other reference to the callable dies here
        gc.collect()
        out = w(torch.zeros(1, 2), torch.tensor([3]), None)
        assert float(out[0, 0]) == 300.0          # step 3 of ddim10 = original timestep 300
    w1, w2 = d._wrap_model(m), d._wrap_model(m)
    w1(torch.zeros(1, 2), torch.tensor([1]), None)
    assert w1._maps is w2._maps and len(w1._maps) == 1
    r = weakref.ref(m)
    del m, w, w1, w2
    gc.collect()
    assert r() is None and len(d._wrapped) == 0


def test_extract_into_tensor_tables_are_keyed_by_content():
    """_extract_into_tensor (gaussian_diffusion.py:850-863 of the reference: from_numpy(arr).to(device)[t].float(), broadcast) keeps one device copy
    per table CONTENT: callers pass temporaries (1.0 - alphas_cumprod) whose addresses the allocator reuses - a second array at the same
    address with other values must not hit the first one's copy - and the values are the reference expression's."""
    import torch
    from humanliff_amd.improved_diffusion import gaussian_diffusion as gd
    t = torch.tensor([0, 3, 999, 500])
    rng = np.random.default_rng(0)
    for _ in range(3):
        arr = rng.random(1000)                      # fp64, like the schedule tables
        got = gd._extract_into_tensor(arr, t, (4, 2, 3))
        ref = torch.from_numpy(arr)[t].float()
        assert got.shape == (4, 2, 3) and torch.equal(got[:, 0, 0], ref) and torch.equal(got[:, 1, 2], ref)
        arr[...] = rng.random(1000)                 # same address, new content
        assert torch.equal(gd._extract_into_tensor(arr, t, (4,)), torch.from_numpy(arr)[t].float())
    arr32 = rng.random(1000).astype(np.float32)     # another dtype with other bytes of the same length is its own entry
    assert torch.equal(gd._extract_into_tensor(arr32, t, (4,)), torch.from_numpy(arr32)[t].float())
    assert len(gd._TABLES) <= 256


def test_bench_line_is_compact():
    """the driver reads ONE JSON line from bench.py's stdout.  Round 5's line had grown to 20 KB and the driver's record came back
    unparsed; `bench_line.compact_line` now reduces everything measured to < 6 KB with no string over 160 characters (the rest goes to
    bench_detail.json).  Canned input: round 5's full result (profiles/r05_bench.json) plus a worst-case synthetic one."""
    import json
    import os
    import bench_line
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full = json.load(open(os.path.join(root, "profiles", "r05_bench.json")))
    line = bench_line.compact_line(full)
    s = json.dumps(line)
    assert len(s) < 8192 and len(s) < bench_line.MAX_LINE_BYTES and "\n" not in s
    assert max(len(x) for x in bench_line._strings(line)) <= 160
    back = json.loads(s)
    assert back == line
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "config", "roofline", "cpu_baseline", "parity", "summary"):
        assert k in back, k
    assert back["value"] == full["value"] and back["metric"] == "denoise-steps/sec" and "workload" in back["config"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in back["roofline"], k
    assert abs(back["roofline"]["frac"] - back["roofline"]["achieved"] / back["roofline"]["peak"]) < 1e-3
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in back["cpu_baseline"], k
    for leg in ("render", "fit"):
        assert set(("value", "unit", "roofline", "cpu_baseline")) <= set(back[leg]), leg
    assert back["render"]["parity"]["psnr_db"] > 45
    # worst case: every string absurdly long, non-finite numbers, an N > 1 run without the N = 1-only legs
    junk = "x" * 5000
    worst = dict(full, dtype_note=junk, cpu_baseline=None, parity=None, e2e=None, train=None,
                 rccl={"world_size": 8, "backend": "nccl", "device_count_visible": 8, "sample_gather": {"recv_gb_per_s_per_rank": float("nan")},
                       "image_gather_uint8": {"recv_gb_per_s_per_rank": 301.5, "note": junk}})
    worst["config"] = dict(full["config"], workload=junk)
    worst["roofline"] = dict(full["roofline"], kernel=junk, note=junk)
    w = bench_line.compact_line(worst)
    ws = json.dumps(w)
    assert len(ws) < bench_line.MAX_LINE_BYTES and json.loads(ws) == w and "NaN" not in ws
    assert w["rccl"]["backend"] == "nccl" and w["rccl"]["image_gather_uint8_recv_gb_per_s_per_rank"] == 301.5


def test_bench_dump_outputs_budget_and_sample(tmp_path):
    """bench.py --dump-outputs: every array as <name>.npy in float32 (float64 kept); within the budget the arrays are written whole, above
    it each one becomes the same seeded sample of its elements, so two runs (two builds) stay comparable array for array."""
    import bench
    g = torch.Generator().manual_seed(3)
    arrays = {"sample": torch.randn((4, 3, 16, 16), generator=g), "pred_xstart": torch.randn((4, 3, 16, 16), generator=g).double(),
              "half": torch.randn((2, 8), generator=g).half()}
    bench.dump_outputs(arrays, str(tmp_path / "whole"))
    for k, v in arrays.items():
        a = np.load(tmp_path / "whole" / f"{k}.npy")
        assert a.dtype == (np.float64 if v.dtype == torch.float64 else np.float32) and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.double().numpy() if v.dtype == torch.float64 else v.float().numpy())
    budget = 4096 * 3 + 8000
    for d in ("cut_a", "cut_b"):
        bench.dump_outputs(arrays, str(tmp_path / d), budget=budget)
    total = 0
    for k, v in arrays.items():
        a, b = np.load(tmp_path / "cut_a" / f"{k}.npy"), np.load(tmp_path / "cut_b" / f"{k}.npy")
        assert a.ndim == 1 and 0 < a.size < v.numel() and np.array_equal(a, b)
        flat = (v.double() if v.dtype == torch.float64 else v.float()).reshape(-1).numpy()
        assert np.isin(a, flat).all()
        total += os.path.getsize(tmp_path / "cut_a" / f"{k}.npy")
    assert total <= budget
