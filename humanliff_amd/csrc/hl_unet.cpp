// Host runtime of the tri-plane UNet denoiser: binds a reference state_dict, packs the weights
// and walks the network issuing the kernels of hl_unet_kernels.hip on the caller's stream.
//
// Mirrors the structure UNetModel.__init__ builds (human_diffusion/improved_diffusion/unet.py:323-525)
// and the dataflow of UNetModel.forward (unet.py:550-615) for cond_type in {"controlnet", ""},
// use_scale_shift_norm=True, dims=2.  Activations are NHWC fp32; every skip "concat" of the decoder is a
// buffer whose two channel ranges are written in place by their producers (the previous decoder block and
// the control-branch zero-conv, whose epilogue also adds the encoder skip: hs.pop() + hs_cond.pop()).
#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "hl_stat_book.h"
#include "hl_unet_kernels.h"
#include <algorithm>

namespace {

using hl::ConvArgs;
using hl::View;

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

using hl::WeightForm;
using hl::conv_forms;
using hl::conv_mode_known;

struct Conv {
    hl::ConvWeights w;   // every packed form the layer has (make_conv_w); a forward uses those of conv_forms(Net::conv_mode)
    const float *bias = nullptr;
    int Cin = 0, Cin_pad = 0, Cout = 0, ks = 1;
};
struct Norm {
    const float *gamma = nullptr, *beta = nullptr;
    int C = 0;
    float eps = 1e-5f;
};
struct Res {
    Norm n1, n2;
    Conv c1, c2, skip;
    bool has_skip = false;
    bool aware = false;   // use_3d_aware: out_layers' conv reads cat[h, two plane means] = 3*Cout channels (unet.py:158-166, 208-214)
    long emb_off = 0;
    int Cin = 0, Cout = 0;
};
struct Attn {
    Norm norm;
    Conv qkv, proj;
    int C = 0, heads = 1;
};
// cond_type='cross_attention': SpatialTransformer (spatial_transformer.py:136-178) in place of AttentionBlock, depth 1
struct Xf {
    Norm norm;                                  // GroupNorm(32, C, eps 1e-6)
    Conv proj_in, proj_out, qkv, out1, ff_in, ff_out;
    const float *ln1_g = nullptr, *ln1_b = nullptr, *ln3_g = nullptr, *ln3_b = nullptr;
    const float *v2_w = nullptr, *o2_w = nullptr, *o2_b = nullptr;   // attn2: to_v (C, E), to_out.0 (C, C) + bias
    int C = 0, heads = 1;
};
enum Kind { K_CONV, K_RES, K_ATTN, K_DOWN, K_UP, K_XF };
struct Layer {
    Kind kind;
    int idx;
};
struct Block {
    std::vector<Layer> layers;
    int Cout = 0;
    int ds_out = 1;  // spatial downsample factor of the block output
};

struct Net {
    hl_unet_cfg cfg{};
    std::unordered_map<std::string, std::pair<const float *, int64_t>> sd;
    std::vector<Conv> convs;  // bare convs, down/up convs, proj convs
    std::vector<Res> res;
    std::vector<Attn> attn;
    std::vector<Xf> xf;
    std::vector<Block> in_blocks, out_blocks, cond_blocks;
    Block middle;
    std::vector<int> proj_cond;  // conv index per control block
    Conv out_conv;
    Norm out_norm;
    const float *te0_w = nullptr, *te0_b = nullptr, *te2_w = nullptr, *te2_b = nullptr, *label = nullptr;
    // cond_type == "AdaGN" (unet.py:519-525, 574-578): x_cond -> conv 3x3 s2 (6) -> conv 3x3 s2 (1) -> Linear(64*64, E), added to emb
    Conv ada1, ada2;
    const float *ada_w = nullptr, *ada_b = nullptr;
    const float *emb_w = nullptr, *emb_b = nullptr;  // stacked emb_layers
    long emb_total = 0;
    int E = 0;         // time_embed_dim
    int Cpad0 = 0;     // padded input channels
    // packing cursor
    float *packed = nullptr;
    size_t packed_off = 0;  // floats
    bool dry = true;        // only size the packed buffer
    hipStream_t st = nullptr;
    std::string err;
    // the control encoder runs on its own stream next to the main encoder (they only meet at the skip sums)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::vector<hipEvent_t> ev_block;   // main encoder block i finished (its output feeds the skip sum)
    bool overlap = true;
    int conv_mode = HL_CONV_FP32;   // HL_CONV_* (hl_unet_set_conv_mode): which of the layers' packed forms a forward may use (hl::conv_forms)
    // optional per-category HIP-event timing of one forward (bench.py roofline leg)
    bool prof = false;
    std::vector<hipEvent_t> ev_pool;
    struct Span { int cat; size_t a, b; double flops, exec; int key[5]; long mid; };   // mid: event between pre-pass and kernel (-1: none)   // algorithmic FLOPs and the FLOPs the kernel actually issued; conv launches: {path, level, Cin, Cout, ks}
    double dom[4] = {0, 0, 0, 0};   // dominant convolution shape of the last profile read: total ms, algorithmic / executed FLOPs per launch, launches
    int dom_key[5] = {0, 0, 0, 0, 0};
    std::vector<Span> spans;
    size_t ev_used = 0;
    // which kernel family each convolution of the LAST forward took, per resolution level (hl_unet_dispatch_census):
    // [hl::conv_census_row(path)][log2(H / H_out)]
    int64_t census[5][8] = {};
    ~Net() {
        for (auto e : ev_pool) if (e) hipEventDestroy(e);
        for (auto e : ev_block) if (e) hipEventDestroy(e);
        if (ev_fork) hipEventDestroy(ev_fork);
        if (ev_join) hipEventDestroy(ev_join);
        if (side) hipStreamDestroy(side);
    }
    size_t next_event() {
        if (ev_used == ev_pool.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) { if (err.empty()) err = "hipEventCreate failed (profiling events)"; e = nullptr; }
            ev_pool.push_back(e);
        }
        return ev_used++;
    }
};
enum { CAT_CONV = 0, CAT_GN = 1, CAT_ATTN = 2, CAT_OTHER = 3, CAT_N = 4 };

const float *lookup(Net &n, const std::string &name, int64_t expect) {
    if (n.dry) return reinterpret_cast<const float *>(16);
    auto it = n.sd.find(name);
    if (it == n.sd.end()) { if (n.err.empty()) n.err = "missing state_dict key: " + name; return nullptr; }
    if (expect >= 0 && it->second.second != expect) {
        if (n.err.empty()) n.err = "shape mismatch for " + name + ": got " + std::to_string(it->second.second) + " elements, expected " + std::to_string(expect);
        return nullptr;
    }
    return it->second.first;
}

// floats a weight form of `bytes` takes in the packed buffer (every form starts on 256 bytes), and all the forms of a layer
size_t form_floats(size_t bytes) { return (bytes / 4 + 63) / 64 * 64; }
size_t conv_forms_floats(int Cout, int Cin_pad, int ks) {
    size_t t = 0;
    for (int f = 0; f < hl::kWeightForms; ++f) t += form_floats(hl::conv_form_bytes((WeightForm)f, Cout, Cin_pad, ks));
    return t;
}
// ups: the convolution of an Upsample layer (it alone has the phase form, WeightForm::Fp16x2Up)
Conv make_conv_w(Net &n, const float *w, const float *bias, int Cin, int Cout, int ks, bool ups = false);
Conv make_conv(Net &n, const std::string &p, int Cin, int Cout, int ks, bool has_bias = true, bool ups = false) {
    const float *w = lookup(n, p + ".weight", (int64_t)Cout * Cin * ks * ks);
    const float *b = has_bias ? lookup(n, p + ".bias", Cout) : nullptr;
    return make_conv_w(n, w, b, Cin, Cout, ks, ups);
}
Conv make_conv_w(Net &n, const float *w, const float *bias, int Cin, int Cout, int ks, bool ups) {
    Conv c;
    c.Cin = Cin; c.Cin_pad = round_up(Cin, 16); c.Cout = Cout; c.ks = ks;
    c.bias = n.dry ? nullptr : bias;
    const int cp = c.Cin_pad;
    // every form the layer has, in buffer order
    for (int f = 0; f < hl::kWeightForms; ++f) {
        const size_t bytes = hl::conv_form_bytes((WeightForm)f, Cout, cp, ks, true, ups);
        if (!bytes) continue;
        float *dst = n.dry ? nullptr : n.packed + n.packed_off;
        n.packed_off += form_floats(bytes);
        if (n.dry || !w) continue;
        c.w.p[f] = dst;
        if (hl::conv_pack_form((WeightForm)f, w, Cout, Cin, cp, ks, dst, n.st) != 0 && n.err.empty()) n.err = hl_last_error();   // (the 16-bit form in fp16: conv_forms)
    }
    return c;
}
Norm make_norm(Net &n, const std::string &p, int C) {
    Norm g;
    g.C = C;
    g.gamma = lookup(n, p + ".weight", C);
    g.beta = lookup(n, p + ".bias", C);
    return g;
}

struct EmbPiece { std::string name; int O; long off; };

int add_res(Net &n, std::vector<EmbPiece> &emb, const std::string &p, int Cin, int Cout, bool aware = false) {
    Res r;
    r.Cin = Cin; r.Cout = Cout; r.aware = aware;
    r.n1 = make_norm(n, p + ".in_layers.0", Cin);
    r.c1 = make_conv(n, p + ".in_layers.2", Cin, Cout, 3);
    r.emb_off = n.emb_total;
    const int emb_o = n.cfg.no_scale_shift ? Cout : 2 * Cout;      // unet.py:186-191
    emb.push_back({p + ".emb_layers.1", emb_o, n.emb_total});
    n.emb_total += emb_o;
    r.n2 = make_norm(n, p + ".out_layers.0", Cout);
    r.c2 = make_conv(n, p + ".out_layers.3", aware ? 3 * Cout : Cout, Cout, 3);
    r.has_skip = Cin != Cout;
    if (r.has_skip) {
        // the shipped config uses a 1x1 skip (use_conv=False, unet.py:177-184); a 3x3 one is told apart by size
        int ks = 1;
        if (!n.dry) {
            auto it = n.sd.find(p + ".skip_connection.weight");
            if (it != n.sd.end() && it->second.second == (int64_t)Cout * Cin * 9) ks = 3;
        }
        r.skip = make_conv(n, p + ".skip_connection", Cin, Cout, ks);
        if (n.dry) {   // sized as 1x1 above: room for the 3x3 one where that is larger
            const size_t f1 = conv_forms_floats(Cout, round_up(Cin, 16), 1), f3 = conv_forms_floats(Cout, round_up(Cin, 16), 3);
            if (f3 > f1) n.packed_off += f3 - f1;
        }
    }
    n.res.push_back(r);
    return (int)n.res.size() - 1;
}
int add_attn(Net &n, const std::string &p, int C, int heads) {
    Attn a;
    a.C = C; a.heads = heads;
    a.norm = make_norm(n, p + ".norm", C);
    a.qkv = make_conv(n, p + ".qkv", C, 3 * C, 1);
    a.proj = make_conv(n, p + ".proj_out", C, C, 1);
    n.attn.push_back(a);
    return (int)n.attn.size() - 1;
}
int add_xf(Net &n, const std::string &p, int C, int heads) {
    Xf a;
    a.C = C; a.heads = heads;
    a.norm = make_norm(n, p + ".norm", C);
    a.norm.eps = 1e-6f;
    a.proj_in = make_conv(n, p + ".proj_in", C, C, 1);
    const std::string t = p + ".transformer_blocks.0";
    // self-attention: to_q / to_k / to_v (no bias; output channel = head*d + c) stacked into ONE projection in the layout the attention
    // kernel reads, channel = head*3d + {q,k,v}*d + c
    const int d = C / heads;
    const float *wq = lookup(n, t + ".attn1.to_q.weight", (int64_t)C * C), *wk = lookup(n, t + ".attn1.to_k.weight", (int64_t)C * C),
                *wv = lookup(n, t + ".attn1.to_v.weight", (int64_t)C * C);
    float *fused = n.dry ? nullptr : n.packed + n.packed_off;
    n.packed_off += ((size_t)3 * C * C + 63) / 64 * 64;
    if (!n.dry && wq && wk && wv) {
        const float *src[3] = {wq, wk, wv};
        for (int h = 0; h < heads; ++h)
            for (int q = 0; q < 3; ++q)
                hipMemcpyAsync(fused + ((size_t)h * 3 + q) * d * C, src[q] + (size_t)h * d * C, (size_t)d * C * sizeof(float), hipMemcpyDeviceToDevice, n.st);
    }
    a.qkv = make_conv_w(n, n.dry ? reinterpret_cast<const float *>(16) : fused, nullptr, C, 3 * C, 1);
    a.out1 = make_conv(n, t + ".attn1.to_out.0", C, C, 1);
    a.ln1_g = lookup(n, t + ".norm1.weight", C); a.ln1_b = lookup(n, t + ".norm1.bias", C);
    a.ln3_g = lookup(n, t + ".norm3.weight", C); a.ln3_b = lookup(n, t + ".norm3.bias", C);
    a.v2_w = lookup(n, t + ".attn2.to_v.weight", (int64_t)C * n.E);
    a.o2_w = lookup(n, t + ".attn2.to_out.0.weight", (int64_t)C * C);
    a.o2_b = lookup(n, t + ".attn2.to_out.0.bias", C);
    a.ff_in = make_conv(n, t + ".ff.net.0.proj", C, 8 * C, 1);
    a.ff_out = make_conv(n, t + ".ff.net.2", 4 * C, C, 1);
    a.proj_out = make_conv(n, p + ".proj_out", C, C, 1);
    n.xf.push_back(a);
    return (int)n.xf.size() - 1;
}
int add_conv(Net &n, const std::string &p, int Cin, int Cout, int ks, bool ups = false) {
    n.convs.push_back(make_conv(n, p, Cin, Cout, ks, true, ups));
    return (int)n.convs.size() - 1;
}
bool has_ds(const hl_unet_cfg &c, int ds) {
    for (int i = 0; i < c.n_attention_ds; ++i)
        if (c.attention_ds[i] == ds) return true;
    return false;
}

// builds one encoder (main or control) following unet.py:375-415 / 477-518
void build_encoder(Net &n, std::vector<EmbPiece> &emb, const std::string &root, std::vector<Block> &blocks,
                   std::vector<int> &chans, bool aware) {
    const hl_unet_cfg &c = n.cfg;
    Block b0;
    b0.layers.push_back({K_CONV, add_conv(n, root + ".0.0", c.in_channels, c.model_channels, 3)});
    b0.Cout = c.model_channels;
    b0.ds_out = 1;
    blocks.push_back(b0);
    chans.push_back(c.model_channels);
    int ch = c.model_channels, ds = 1, bi = 1;
    for (int level = 0; level < c.n_levels; ++level) {
        for (int r = 0; r < c.num_res_blocks; ++r) {
            Block b;
            const std::string p = root + "." + std::to_string(bi);
            const int co = c.channel_mult[level] * c.model_channels;
            b.layers.push_back({K_RES, add_res(n, emb, p + ".0", ch, co, aware)});
            ch = co;
            if (has_ds(c, ds)) {
                if (c.cross_attn) b.layers.push_back({K_XF, add_xf(n, p + ".1", ch, c.num_heads)});
                else b.layers.push_back({K_ATTN, add_attn(n, p + ".1", ch, c.num_heads)});
            }
            b.Cout = ch; b.ds_out = ds;
            blocks.push_back(b);
            chans.push_back(ch);
            ++bi;
        }
        if (level != c.n_levels - 1) {
            Block b;
            const std::string p = root + "." + std::to_string(bi);
            b.layers.push_back({K_DOWN, add_conv(n, p + ".0.op", ch, ch, 3)});
            ds *= 2;
            b.Cout = ch; b.ds_out = ds;
            blocks.push_back(b);
            chans.push_back(ch);
            ++bi;
        }
    }
}

void build(Net &n) {
    const hl_unet_cfg &c = n.cfg;
    n.E = 4 * c.model_channels;
    n.Cpad0 = round_up(c.in_channels, 16);
    n.emb_total = 0;
    n.packed_off = 0;
    n.convs.clear(); n.res.clear(); n.attn.clear(); n.xf.clear();
    n.in_blocks.clear(); n.out_blocks.clear(); n.cond_blocks.clear(); n.proj_cond.clear();
    std::vector<EmbPiece> emb;
    n.te0_w = lookup(n, "time_embed.0.weight", (int64_t)n.E * c.model_channels);
    n.te0_b = lookup(n, "time_embed.0.bias", n.E);
    n.te2_w = lookup(n, "time_embed.2.weight", (int64_t)n.E * n.E);
    n.te2_b = lookup(n, "time_embed.2.bias", n.E);
    n.label = c.num_classes > 0 ? lookup(n, "label_emb.weight", (int64_t)c.num_classes * n.E) : nullptr;
    if (c.adagn || c.cross_attn) {
        n.ada1 = make_conv(n, "conv_proj_1", c.out_channels, 6, 3);
        n.ada2 = make_conv(n, "conv_proj_2", 6, 1, 3);
        n.ada_w = lookup(n, "linear.weight", (int64_t)n.E * 4096);
        n.ada_b = lookup(n, "linear.bias", n.E);
    }

    std::vector<int> chans;
    const bool aware = c.aware3d != 0;
    build_encoder(n, emb, "input_blocks", n.in_blocks, chans, aware);
    int ch = chans.back();
    int ds = n.in_blocks.back().ds_out;
    {
        Block m;
        m.layers.push_back({K_RES, add_res(n, emb, "middle_block.0", ch, ch, aware)});
        if (c.cross_attn) m.layers.push_back({K_XF, add_xf(n, "middle_block.1", ch, c.num_heads)});
        else m.layers.push_back({K_ATTN, add_attn(n, "middle_block.1", ch, c.num_heads)});
        m.layers.push_back({K_RES, add_res(n, emb, "middle_block.2", ch, ch, aware)});
        m.Cout = ch; m.ds_out = ds;
        n.middle = m;
    }
    std::vector<int> stack = chans;
    int bi = 0;
    for (int level = c.n_levels - 1; level >= 0; --level) {
        for (int i = 0; i <= c.num_res_blocks; ++i) {
            Block b;
            const std::string p = "output_blocks." + std::to_string(bi);
            const int skip = stack.back();
            stack.pop_back();
            const int co = c.model_channels * c.channel_mult[level];
            int li = 0;
            b.layers.push_back({K_RES, add_res(n, emb, p + "." + std::to_string(li++), ch + skip, co, aware)});
            ch = co;
            if (has_ds(c, ds)) {
                if (c.cross_attn) b.layers.push_back({K_XF, add_xf(n, p + "." + std::to_string(li++), ch, c.num_heads)});   // unet.py:463: num_heads
                else b.layers.push_back({K_ATTN, add_attn(n, p + "." + std::to_string(li++), ch, c.num_heads_upsample)});
            }
            if (level && i == c.num_res_blocks) {
                b.layers.push_back({K_UP, add_conv(n, p + "." + std::to_string(li++) + ".conv", ch, ch, 3, true)});
                ds /= 2;
            }
            b.Cout = ch; b.ds_out = ds;
            n.out_blocks.push_back(b);
            ++bi;
        }
    }
    n.out_norm = make_norm(n, "out.0", ch);
    n.out_conv = make_conv(n, "out.2", c.model_channels, c.out_channels, 3);
    if (c.controlnet) {
        std::vector<int> cch;
        build_encoder(n, emb, "input_blocks_cond", n.cond_blocks, cch, false);   // the control tower's ResBlocks are plain (unet.py:477-518)
        for (size_t i = 0; i < n.cond_blocks.size(); ++i)
            n.proj_cond.push_back(add_conv(n, "input_blocks_proj_cond." + std::to_string(i), cch[i], cch[i], 1));
    }
    // stacked emb_layers: rows [emb_total][E] then bias [emb_total]
    const size_t wfl = (size_t)n.emb_total * n.E;
    if (!n.dry) {
        float *wdst = n.packed + n.packed_off, *bdst = wdst + wfl;
        for (auto &e : emb) {
            const float *w = lookup(n, e.name + ".weight", (int64_t)e.O * n.E);
            const float *b = lookup(n, e.name + ".bias", e.O);
            if (!w || !b) continue;
            hipMemcpyAsync(wdst + (size_t)e.off * n.E, w, (size_t)e.O * n.E * sizeof(float), hipMemcpyDeviceToDevice, n.st);
            hipMemcpyAsync(bdst + e.off, b, (size_t)e.O * sizeof(float), hipMemcpyDeviceToDevice, n.st);
        }
        n.emb_w = wdst; n.emb_b = bdst;
    }
    n.packed_off += (wfl + n.emb_total + 63) / 64 * 64;
}

// ---- forward ------------------------------------------------------------------------------------
// the affine of a GroupNorm in front of a convolution: arrays (cA, cB) or - no launch - the producers' group statistics (gn.gs0 set)
struct Aff { float *cA = nullptr, *cB = nullptr; hl::GnSrc gn{}; };
// everything about one convolution call beyond layer, input and output; the defaults are a bare stride-1 convolution that leaves statistics
struct ConvOpt {
    int stride = 1, ups = 0;
    Aff af{};                                            // GroupNorm in front
    int act = 0;                                         // SiLU behind the GroupNorm
    const float *res = nullptr; long res_pitch = 0;      // out = conv + res
    float *out2 = nullptr; long out2_pitch = 0;          // second store out2 = conv + res2 (the control tower's zero-convolution)
    const float *res2 = nullptr; long res2_pitch = 0;
    int nchw = 0;                                        // the network's output layout
    bool stats = true;                                   // add the output's GroupNorm statistics (false: nobody normalises this store)
    void residual(const View &v) { res = v.p; res_pitch = v.pitch; }
};
// a stream and the scratch its launches use.  act_ws: materialised GroupNorm(+SiLU) inputs (k_conv_dma path)
struct Lane { hipStream_t st; float *gn_scratch, *splitk_ws, *act_ws; };

struct Exec {
    Net &n;
    bool run;          // false: only size the workspace
    char *ws;
    int B, H, W;
    size_t off = 0;
    float *emb_all = nullptr;
    const float *ctx = nullptr;    // cond_type='cross_attention': the context token (B, E)
    Lane lanes[2]{};               // the caller's stream, and the side stream of the control tower
    Lane *lane = &lanes[0];        // the one the walk enqueues on
    size_t act_need = 0;           // floats, largest normalised conv input seen
    int rc = 0;
    // GroupNorm statistics travel from the kernel that stores a tensor to the layer that normalises it (ConvArgs::stats); the book says
    // whose totals a consumer may read (hl_stat_book.h, run pass only)
    hl::StatBook book;
    // the fixed-point totals live in one arena behind the activation scratch, zeroed by ONE memset at the start of the forward
    char *stat_base = nullptr;
    size_t stat_off = 0, stat_bytes = 0;
    float *alloc_stat(size_t floats) {
        float *p = run ? reinterpret_cast<float *>(stat_base + stat_off) : nullptr;
        stat_off += (floats * sizeof(float) + 255) / 256 * 256;
        return p;
    }
    // the block an output adds its statistics into: the shared one of a concat half (run pass), else a new one (every output of the sizing pass)
    hl::StatBook::Block stat_block(const float *out, int Cout, long HW) {
        return book.block_for(out, Cout, book.in_concat(out) ? nullptr : alloc_stat(hl::conv_stats_floats(B, HW)));
    }
    Exec(Net &n_, bool run_, char *ws_, hipStream_t st, int B_, int H_, int W_) : n(n_), run(run_), ws(ws_), B(B_), H(H_), W(W_) {
        lanes[0].st = st;
        lanes[1].st = n.side;
    }

    float *alloc(size_t floats) {
        float *p = run ? reinterpret_cast<float *>(ws + off) : nullptr;
        off += (floats * sizeof(float) + 255) / 256 * 256;
        return p;
    }
    View plain(int ds, int C) {
        View v;
        v.N = B; v.H = H / ds; v.W = W / ds; v.C = C; v.pitch = C;
        v.p = alloc((size_t)v.pixels() * C);
        return v;
    }
    void ok(int r) { if (r && !rc) rc = r; }
    size_t span_begin() {
        if (!n.prof) return 0;
        const size_t a = n.next_event();
        if (n.ev_pool[a]) hipEventRecord(n.ev_pool[a], lane->st);
        return a;
    }
    void span_end(int cat, size_t a, double flops, double exec = -1.0) {
        if (!n.prof) return;
        if (!n.err.empty() && !rc) rc = hl::fail(HL_ERR_RUNTIME, "hl_unet_forward: %s", n.err.c_str());
        const size_t b = n.next_event();
        if (n.ev_pool[b]) hipEventRecord(n.ev_pool[b], lane->st);
        n.spans.push_back({cat, a, b, flops, exec < 0 ? flops : exec, {span_key[0], span_key[1], span_key[2], span_key[3], span_key[4]}, span_mid});
        span_key[0] = -1; span_mid = -1;
    }
    int span_key[5] = {-1, 0, 0, 0, 0};
    long span_mid = -1;

    void conv(const Conv &c, const View &in, const View &out, const ConvOpt &o = {}) {
        if (!run) {   // sizing pass (pointers are null here): the largest conv input is also the largest normalised one
            const size_t need = (size_t)in.pixels() * c.Cin_pad;
            if (need > act_need) act_need = need;
        }
        // where the output statistics go (same allocations in the sizing pass)
        hl::StatBook::Block s1{nullptr, c.Cout, 0}, s2{nullptr, c.Cout, 0};
        if (o.stats && !o.nchw) {
            s1 = stat_block(out.p, c.Cout, (long)out.H * out.W);
            if (o.out2_pitch != 0) s2 = stat_block(o.out2, c.Cout, (long)out.H * out.W);
        }
        if (!run) return;
        ConvArgs a{};
        a.in = in; a.in.C = c.Cin_pad;
        a.w = c.w.only(conv_forms(n.conv_mode, false, false)); a.mode = n.conv_mode;
        a.bias = c.bias; a.Cout = c.Cout; a.ks = c.ks; a.stride = o.stride; a.ups = o.ups;
        a.coefA = o.af.cA; a.coefB = o.af.cB; a.act = o.act; a.gn = o.af.gn;
        a.out = out; a.res = o.res; a.res_pitch = o.res_pitch;
        a.out2 = o.out2; a.out2_pitch = o.out2_pitch; a.res2 = o.res2; a.res2_pitch = o.res2_pitch; a.out_nchw = o.nchw;
        a.splitk_ws = lane->splitk_ws; a.splitk_ws_bytes = hl::conv_splitk_ws_bytes();
        a.act_ws = lane->act_ws; a.act_ws_bytes = act_need * sizeof(float);
        a.stats = s1.buf; a.stats2 = s2.buf;
        if (raw_input(o)) a.in_stats = book.totals_of(in.p, in.C, false);     // (the fp16x2 kernels scale a raw input by a power of two from its sum x^2)
        a.st_cg = s1.viewC / 32; a.st_c0 = s1.c0; a.st2_cg = s2.viewC / 32; a.st2_c0 = s2.c0;
        const size_t e0 = span_begin();
        size_t emid = 0;
        if (n.prof) { emid = n.next_event(); a.ev_mid = n.ev_pool[emid]; }
        const hl::ConvPlan pl = hl::plan_conv(a);
        ok(hl::conv2d(a, pl, lane->st));
        note_conv(c, in, out, o, a, pl, e0, emid);
        // whoever stored the tensor last owns its statistics
        if (pl.stat_slots > 0) {
            book.produced(out.p, s1, c.Cout);
            if (o.out2) book.produced(o.out2, s2, c.Cout);
        } else {
            book.stored_without_totals(out.p);
            if (o.out2) book.stored_without_totals(o.out2);
        }
    }
    static bool raw_input(const ConvOpt &o) { return o.af.cA == nullptr && o.af.gn.gt == nullptr; }
    // what a launched convolution leaves outside the network: the developer audit line, the dispatch census, the profiling span
    void note_conv(const Conv &c, const View &in, const View &out, const ConvOpt &o, const ConvArgs &a, const hl::ConvPlan &pl, size_t e0, size_t emid) {
        // developer audit (HL_AUDIT_SCALE=1, read once): fp16x2 launches whose raw input came without totals - their activation planes are unscaled (sx = 1)
        static const int audit_ = [] { const char *e_ = getenv("HL_AUDIT_SCALE"); return e_ ? atoi(e_) : 0; }();
        if (audit_ && pl.path == hl::ConvPath::Fp16x2 && raw_input(o) && a.in_stats == nullptr)
            fprintf(stderr, "[hl audit] fp16x2 convolution with an unscaled raw input: %dx%d px, %d -> %d channels, ks %d, stride %d\n", in.H, in.W, in.C, c.Cout, c.ks, o.stride);
        if (n.prof && a.ev_mid && pl.pre != hl::ConvPrePass::None) span_mid = (long)emid;
        int lvl = 0;
        while (lvl < 7 && (out.H << lvl) < H) ++lvl;
        n.census[hl::conv_census_row(pl.path)][lvl] += 1;
        // (keyed like a rocprofv3 per-kernel, per-grid row: kernel family, level, Cout, kernel size - the input channel counts of a level share a row)
        span_key[0] = (int)pl.path; span_key[1] = lvl; span_key[2] = o.ups ? 1 : 0; span_key[3] = c.Cout; span_key[4] = c.ks;
        const double fl = 2.0 * (double)out.pixels() * c.Cout * c.Cin * c.ks * c.ks;
        span_end(CAT_CONV, e0, fl, fl * hl::conv_issued_factor(pl.path) * (pl.kernel == hl::ConvKernel::H2sUp ? 4.0 / 9.0 : 1.0));   // (four of the nine taps)
    }
    // force_arrays: the caller needs cA / cB in memory (gn_apply_3d)
    Aff coef(const View &x, const Norm &g, const float *emb, bool force_arrays = false) {
        Aff af;
        af.cA = alloc((size_t)B * x.C);
        af.cB = alloc((size_t)B * x.C);
        if (!run) return af;
        const float *gt = book.totals_of(x.p, x.C, true);   // else one pass over the tensor
        if (gt && !force_arrays && !n.prof) {
            // the consumer kernels form the coefficients themselves from the totals the producers left: no launch here
            af.cA = af.cB = nullptr;
            af.gn.gt = gt; af.gn.C = x.C; af.gn.HW = x.H * x.W;
            af.gn.gamma = g.gamma; af.gn.beta = g.beta; af.gn.emb = emb; af.gn.emb_pitch = n.emb_total; af.gn.eps = g.eps;
            return af;
        }
        const size_t e0 = span_begin();
        if (gt) ok(hl::groupnorm_coef_stats(x, gt, g.gamma, g.beta, emb, n.emb_total, af.cA, af.cB, lane->st, g.eps));
        else ok(hl::groupnorm_coef(x, g.gamma, g.beta, emb, n.emb_total, af.cA, af.cB, lane->gn_scratch, lane->st, nullptr, g.eps));
        span_end(CAT_GN, e0, 0.0);
        return af;
    }
    void res_block(const Res &r, const View &x, const View &dst) {
        // use_scale_shift_norm=False (unet.py:216-218): h = h + emb_out[..., None, None]; h = out_layers(h).  The sum is materialised in
        // place and its GroupNorm statistics come from a pass over the tensor (the producer's epilogue saw h without the embedding)
        const bool noss = n.cfg.no_scale_shift;
        ConvOpt o1, o2;
        o1.af = coef(x, r.n1, nullptr); o1.act = 1; o1.stats = !noss;
        View h = plain(H / dst.H, r.Cout), in2 = h;
        conv(r.c1, x, h, o1);
        if (noss && run) ok(hl::add_rowvec(h, emb_all + r.emb_off, lane->st, n.emb_total));
        const Aff a2 = coef(h, r.n2, run && !noss ? emb_all + r.emb_off : nullptr, r.aware);
        if (r.aware) {
            // unet.py:208-214: every plane sees, next to its own normalised features, the other two planes averaged along the axis
            // it does not share with them; materialised (with the SiLU of out_layers) as a 3C-channel tensor for the convolution
            in2 = plain(H / dst.H, 3 * r.Cout);
            float *sums = alloc((size_t)B * 3 * (h.H + h.W / 3) * r.Cout);
            if (run) {
                const size_t e0 = span_begin();
                ok(hl::gn_apply_3d(h, a2.cA, a2.cB, sums, in2.p, lane->st));
                span_end(CAT_GN, e0, 0.0);
            }
        } else {
            o2.af = a2; o2.act = 1;
        }
        if (r.has_skip) {
            ConvOpt sk;
            sk.stats = false;            // dst is finished by c2 below
            conv(r.skip, x, dst, sk);
        }
        o2.residual(r.has_skip ? dst : x);
        conv(r.c2, in2, dst, o2);
    }
    void attn_block(const Attn &a, const View &x, const View &dst) {
        ConvOpt oq, op;
        oq.af = coef(x, a.norm, nullptr);
        oq.stats = false;                // qkv is not normalised
        View qkv = plain(H / x.H, 3 * a.C);
        conv(a.qkv, x, qkv, oq);
        View o = plain(H / x.H, a.C);
        // the attention's output is the RAW input of the projection convolution: the key-split kernels leave its sum x^2 like any other producer (hl_stats.h)
        float *ost = alloc_stat(hl::conv_stats_floats(B, (long)x.H * x.W));
        if (run) {
            const size_t e0 = span_begin();
            int emitted = 0;
            ok(hl::attention(qkv.p, B, x.H * x.W, a.C, a.heads, o.p, lane->st, n.conv_mode == HL_CONV_FP32, ost, &emitted));
            if (emitted) book.produced(o.p, {ost, a.C, 0}, a.C); else book.stored_without_totals(o.p);
            const double T = (double)x.H * x.W;
            span_end(CAT_ATTN, e0, 4.0 * B * T * T * a.C);
        }
        op.residual(x);
        conv(a.proj, o, dst, op);
    }
    // SpatialTransformer (spatial_transformer.py:136-178, BasicTransformerBlock :115-134), depth 1, context = ONE token per image:
    //   h = proj_in(GroupNorm(x));  h += to_out(self-attention(LayerNorm1(h)));  h += to_out2(to_v2(context))  [softmax over a single key
    //   is 1, so norm2 / to_q / to_k of attn2 cannot act];  h += ff_out(GEGLU(ff_in(LayerNorm3(h))));  y = proj_out(h) + x
    void xf_block(const Xf &a, const View &x, const View &dst) {
        const int ds = H / x.H;
        hipStream_t st = lane->st;
        ConvOpt inner;
        inner.stats = false;             // nothing in here feeds a GroupNorm: every call but proj_out
        ConvOpt p_in = inner, p_out1 = inner, p_ff = inner, p_out;
        p_in.af = coef(x, a.norm, nullptr);
        View h = plain(ds, a.C), ln = plain(ds, a.C), qkv = plain(ds, 3 * a.C), o = plain(ds, a.C), h1 = plain(ds, a.C);
        View ln3 = plain(ds, a.C), f8 = plain(ds, 8 * a.C), f4 = plain(ds, 4 * a.C), h2 = plain(ds, a.C);
        float *v2 = alloc((size_t)B * a.C), *r2 = alloc((size_t)B * a.C);
        p_out1.residual(h); p_ff.residual(h1); p_out.residual(x);
        conv(a.proj_in, x, h, p_in);
        if (run) ok(hl::layernorm(h, a.ln1_g, a.ln1_b, ln.p, st));
        conv(a.qkv, ln, qkv, inner);
        if (run) {
            const size_t e0 = span_begin();
            ok(hl::attention(qkv.p, B, x.H * x.W, a.C, a.heads, o.p, st, n.conv_mode == HL_CONV_FP32));
            const double T = (double)x.H * x.W;
            span_end(CAT_ATTN, e0, 4.0 * B * T * T * a.C);
        }
        conv(a.out1, o, h1, p_out1);
        if (run) {
            ok(hl::linear_small(ctx, n.E, B, n.E, a.v2_w, nullptr, a.C, 0, nullptr, nullptr, v2, a.C, st));
            ok(hl::linear_small(v2, a.C, B, a.C, a.o2_w, a.o2_b, a.C, 0, nullptr, nullptr, r2, a.C, st));
            ok(hl::add_rowvec(h1, r2, st));
            ok(hl::layernorm(h1, a.ln3_g, a.ln3_b, ln3.p, st));
        }
        conv(a.ff_in, ln3, f8, inner);
        if (run) ok(hl::geglu(f8.p, f8.pixels(), 4 * a.C, f4.p, st));
        conv(a.ff_out, f4, h2, p_ff);
        conv(a.proj_out, h2, dst, p_out);
    }
    // run one TimestepEmbedSequential; the last layer writes into dst
    void block(const Block &b, View x, const View &dst) {
        for (size_t i = 0; i < b.layers.size(); ++i) {
            const Layer &L = b.layers[i];
            const bool last = i + 1 == b.layers.size();
            int Cout, ds_out;
            const int ds_in = H / x.H;
            switch (L.kind) {
                case K_CONV: Cout = n.convs[L.idx].Cout; ds_out = ds_in; break;
                case K_RES: Cout = n.res[L.idx].Cout; ds_out = ds_in; break;
                case K_ATTN: Cout = n.attn[L.idx].C; ds_out = ds_in; break;
                case K_XF: Cout = n.xf[L.idx].C; ds_out = ds_in; break;
                case K_DOWN: Cout = n.convs[L.idx].Cout; ds_out = ds_in * 2; break;
                default: Cout = n.convs[L.idx].Cout; ds_out = ds_in / 2; break;
            }
            View y = last ? dst : plain(ds_out, Cout);
            ConvOpt o;
            switch (L.kind) {
                case K_CONV: conv(n.convs[L.idx], x, y); break;
                case K_RES: res_block(n.res[L.idx], x, y); break;
                case K_ATTN: attn_block(n.attn[L.idx], x, y); break;
                case K_XF: xf_block(n.xf[L.idx], x, y); break;
                case K_DOWN: o.stride = 2; conv(n.convs[L.idx], x, y, o); break;
                case K_UP: o.ups = 1; conv(n.convs[L.idx], x, y, o); break;
            }
            x = y;
        }
    }

    void forward(const float *x, const int64_t *t, const float *tf, const float *x_cond, const int64_t *y, float *out) {
        const hl_unet_cfg &c = n.cfg;
        hipStream_t st = lane->st;     // the caller's stream: everything in here but the control tower
        if (run && stat_bytes) ok(hipMemsetAsync(stat_base, 0, stat_bytes, st) == hipSuccess ? 0 : hl::fail(HL_ERR_RUNTIME, "hl_unet_forward: memset of the statistics arena"));
        for (Lane &l : lanes) {
            l.gn_scratch = alloc(hl::gn_scratch_floats(B));
            l.splitk_ws = alloc(hl::conv_splitk_ws_bytes() / sizeof(float));
        }
        // embeddings (unet.py:564, 584-586) and all ResBlock emb_layers in one stacked product
        float *temb = alloc((size_t)B * c.model_channels), *e1 = alloc((size_t)B * n.E), *emb = alloc((size_t)B * n.E);
        emb_all = alloc((size_t)B * n.emb_total);
        View xin; xin.N = B; xin.H = H; xin.W = W; xin.C = n.Cpad0; xin.pitch = n.Cpad0;
        xin.p = alloc((size_t)xin.pixels() * n.Cpad0);
        View xsum = xin;
        if (c.controlnet) xsum.p = alloc((size_t)xin.pixels() * n.Cpad0);
        // the inputs' sum x^2 per image (k_prep_inputs): the activation scale of the two 27 -> 192 input convolutions
        float *xin_tot = alloc_stat(hl::conv_stats_floats(B, (long)H * W)), *xsum_tot = alloc_stat(hl::conv_stats_floats(B, (long)H * W));
        // AdaGN: the condition is projected to one more summand of emb (unet.py:574-578): two stride-2 convs, then a Linear over the
        // 64x64 map (so H = W = 256, as in the reference).  emb = (time_embed + label_emb[y]) + projection.
        View ac, a1, a2;
        float *emb0 = nullptr;
        int64_t *iota = nullptr;
        if (c.adagn || c.cross_attn) {
            ac.N = B; ac.H = H; ac.W = W; ac.C = round_up(c.out_channels, 16); ac.pitch = ac.C; ac.p = alloc((size_t)ac.pixels() * ac.C);
            a1.N = B; a1.H = H / 2; a1.W = W / 2; a1.C = 16; a1.pitch = 16; a1.p = alloc((size_t)a1.pixels() * 16);
            a2.N = B; a2.H = H / 4; a2.W = W / 4; a2.C = 1; a2.pitch = 1; a2.p = alloc((size_t)a2.pixels());
            emb0 = alloc((size_t)B * n.E);
            iota = reinterpret_cast<int64_t *>(alloc(2 * 16));
            if (run) {
                static const int64_t h_iota[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
                ok(hipMemcpyAsync(iota, h_iota, sizeof(h_iota), hipMemcpyHostToDevice, st) == hipSuccess ? 0 : hl::fail(HL_ERR_RUNTIME, "hl_unet_forward: memcpy"));
                ok(hipMemsetAsync(a1.p, 0, (size_t)a1.pixels() * 16 * sizeof(float), st) == hipSuccess ? 0 : hl::fail(HL_ERR_RUNTIME, "hl_unet_forward: memset"));
                ok(hl::prep_inputs(x_cond, nullptr, B, c.out_channels, H, W, ac.C, ac.p, nullptr, st));
            }
            View a1w = a1; a1w.C = 6;                                 // the conv writes 6 of the 16 (zeroed) channels
            ConvOpt down;
            down.stride = 2;
            conv(n.ada1, ac, a1w, down);
            conv(n.ada2, a1, a2, down);
        }
        if (run) {
            const size_t e0 = span_begin();
            ok(hl::timestep_embedding(t, tf, B, c.model_channels, temb, st));
            ok(hl::linear_small(temb, c.model_channels, B, c.model_channels, n.te0_w, n.te0_b, n.E, 0, nullptr, nullptr, e1, n.E, st));
            ok(hl::linear_small(e1, n.E, B, n.E, n.te2_w, n.te2_b, n.E, 1, c.num_classes > 0 ? n.label : nullptr, y, c.adagn ? emb0 : emb, n.E, st));
            ctx = emb0;
            if (c.adagn) ok(hl::linear_small(a2.p, 4096, B, 4096, n.ada_w, n.ada_b, n.E, 0, emb0, iota, emb, n.E, st));
            if (c.cross_attn) ok(hl::linear_small(a2.p, 4096, B, 4096, n.ada_w, n.ada_b, n.E, 0, nullptr, nullptr, emb0, n.E, st));   // the context token (unet.py:579-582)
            ok(hl::linear_small(emb, n.E, B, n.E, n.emb_w, n.emb_b, (int)n.emb_total, 1, nullptr, nullptr, emb_all, n.emb_total, st));
            if (c.aware3d) ok(hl::prep_inputs_3d(x, c.controlnet ? x_cond : nullptr, B, c.in_channels, H, W / 3, n.Cpad0, xin.p,
                                                 c.controlnet ? xsum.p : nullptr, st));
            else {
                ok(hl::prep_inputs(x, c.controlnet ? x_cond : nullptr, B, c.in_channels, H, W, n.Cpad0, xin.p,
                                   c.controlnet ? xsum.p : nullptr, st, xin_tot, c.controlnet ? xsum_tot : nullptr));
                book.produced(xin.p, {xin_tot, n.Cpad0, 0}, n.Cpad0);
                if (c.controlnet) book.produced(xsum.p, {xsum_tot, n.Cpad0, 0}, n.Cpad0);
            }
            span_end(CAT_OTHER, e0, 2.0 * B * ((double)n.E * c.model_channels + (double)n.E * n.E + (double)n.emb_total * n.E));
        }
        // decoder "concat" buffers: [h | skip]; sized from the block structure
        const size_t nb = n.in_blocks.size();
        std::vector<View> cat(nb);
        {
            int ch = n.middle.Cout;
            for (size_t j = 0; j < nb; ++j) {
                const Block &src = n.in_blocks[nb - 1 - j];
                cat[j] = plain(src.ds_out, ch + src.Cout);
                ch = n.out_blocks[j].Cout;
            }
        }
        // one statistics block per concat view, shared by its two halves (the decoder's running tensor | encoder skip + control residual)
        {
            int ch = n.middle.Cout;
            for (size_t j = 0; j < nb; ++j) {
                float *cat_st = alloc_stat(hl::conv_stats_floats(B, (long)cat[j].H * cat[j].W));
                if (run && c.controlnet) book.concat_halves(cat[j].p, cat[j].C, ch, cat_st);
                ch = n.out_blocks[j].Cout;
            }
        }
        auto first_part = [&](size_t j, int C) { View v = cat[j]; v.C = C; return v; };
        // main encoder + middle on the caller's stream; control encoder on the side stream (unet.py:588-602).
        // They are independent except that control block i's zero-conv adds the main encoder's hs[i].
        const bool fork = run && c.controlnet && n.overlap && !n.prof && n.side;
        if (fork) {
            hipEventRecord(n.ev_fork, st);
            hipStreamWaitEvent(n.side, n.ev_fork, 0);
        }
        std::vector<View> hs(nb);
        View h = xin;
        for (size_t i = 0; i < nb; ++i) {
            hs[i] = plain(n.in_blocks[i].ds_out, n.in_blocks[i].Cout);
            block(n.in_blocks[i], h, hs[i]);
            if (fork) hipEventRecord(n.ev_block[i], st);
            h = hs[i];
        }
        block(n.middle, h, first_part(0, n.middle.Cout));
        // control branch: zero-conv output feeds the next block AND (+ encoder skip) the decoder
        if (c.controlnet) {
            if (fork) lane = &lanes[1];
            View hc = xsum;
            for (size_t i = 0; i < nb; ++i) {
                View tmp = plain(n.cond_blocks[i].ds_out, n.cond_blocks[i].Cout);
                block(n.cond_blocks[i], hc, tmp);
                View pj = plain(n.cond_blocks[i].ds_out, n.cond_blocks[i].Cout);
                const size_t j = nb - 1 - i;
                const int Ch = cat[j].C - hs[i].C;
                if (fork) hipStreamWaitEvent(n.side, n.ev_block[i], 0);
                ConvOpt zo;
                zo.out2 = run ? cat[j].p + Ch : nullptr; zo.out2_pitch = cat[j].pitch; zo.res2 = hs[i].p; zo.res2_pitch = hs[i].pitch;
                conv(n.convs[n.proj_cond[i]], tmp, pj, zo);
                hc = pj;
            }
            if (fork) {
                hipEventRecord(n.ev_join, n.side);
                lane = &lanes[0];
                hipStreamWaitEvent(st, n.ev_join, 0);
            }
        } else if (run) {
            for (size_t i = 0; i < nb; ++i) {
                const size_t j = nb - 1 - i;
                const int Ch = cat[j].C - hs[i].C;
                hipMemcpy2DAsync(cat[j].p + Ch, cat[j].pitch * sizeof(float), hs[i].p, hs[i].pitch * sizeof(float),
                                 (size_t)hs[i].C * sizeof(float), (size_t)hs[i].pixels(), hipMemcpyDeviceToDevice, st);
                book.stored_without_totals(cat[j].p + Ch);   // (the source's totals are grouped for its own norm, not for the concat: the decoder norm takes a pass over the tensor)
            }
        }
        // decoder
        View last;
        for (size_t j = 0; j < nb; ++j) {
            View dst = (j + 1 < nb) ? first_part(j + 1, n.out_blocks[j].Cout) : plain(n.out_blocks[j].ds_out, n.out_blocks[j].Cout);
            block(n.out_blocks[j], cat[j], dst);
            last = dst;
        }
        ConvOpt oo;
        oo.af = coef(last, n.out_norm, nullptr); oo.act = 1; oo.nchw = 1;
        View o; o.N = B; o.H = H; o.W = W; o.C = c.out_channels; o.pitch = c.out_channels; o.p = out;
        if (c.aware3d) o.p = alloc((size_t)o.pixels() * c.out_channels);   // unet.py:613-614: the planes go back to channels
        conv(n.out_conv, last, o, oo);
        if (c.aware3d && run) ok(hl::unroll_planes(o.p, B, c.out_channels, H, W / 3, out, st));
    }
};

// The workspace from the sizing pass's results: | bump region (off) | act_ws of lane 0 | act_ws of lane 1 | statistics arena (stat_off) |, byte
// offsets.  The arena starts on a 256-byte ADDRESS, so its offset depends on where the workspace lies (base; 0 in the size query).  The
// total is what hl_unet_workspace_bytes has always returned; its 1024 holds the two round-ups wherever the workspace lies.
struct WsLayout { size_t act_ws[2], stats, total; };
int ws_layout(size_t off, size_t act_need, size_t stat_off, uintptr_t base, WsLayout *L) {
    const size_t act = act_need * sizeof(float);
    L->act_ws[0] = (off + 255) / 256 * 256;
    L->act_ws[1] = L->act_ws[0] + act;
    const size_t end = L->act_ws[1] + act;
    L->stats = end + ((256 - ((base + end) & 255)) & 255);
    L->total = off + 2 * act + stat_off + 1024;
    HL_REQUIRE(L->stats + stat_off <= L->total, "hl_unet: the statistics arena ends %zu bytes behind the workspace", L->stats + stat_off - L->total);
    return 0;
}

int validate(const hl_unet_cfg *c) {
    HL_REQUIRE(c, "unet: null cfg");
    HL_REQUIRE(c->n_levels >= 1 && c->n_levels <= 8 && c->n_attention_ds >= 0 && c->n_attention_ds <= 8, "unet: bad cfg sizes");
    HL_REQUIRE(c->model_channels % 32 == 0, "unet: model_channels must be a multiple of 32 (GroupNorm32)");
    HL_REQUIRE(c->in_channels > 0 && c->out_channels > 0 && c->num_res_blocks > 0 && c->num_heads > 0, "unet: bad cfg");
    HL_REQUIRE(!(c->controlnet && c->adagn), "unet: cond_type is either controlnet or AdaGN");
    HL_REQUIRE(!(c->aware3d && (c->adagn || c->cross_attn)), "unet: use_3d_aware with cond_type='AdaGN' / 'cross_attention' is not built");
    HL_REQUIRE(c->controlnet + c->adagn + c->cross_attn <= 1, "unet: one cond_type");
    return 0;
}

}  // namespace

extern "C" {

size_t hl_unet_packed_bytes(const hl_unet_cfg *cfg) {
    if (validate(cfg)) return 0;
    Net n;
    n.cfg = *cfg;
    if (n.cfg.num_heads_upsample <= 0) n.cfg.num_heads_upsample = n.cfg.num_heads;
    n.dry = true;
    build(n);
    return n.packed_off * sizeof(float) + 256;
}

int hl_unet_create(const hl_unet_cfg *cfg, int n_tensors, const char *const *names, const void *const *ptrs,
                   const int64_t *numels, void *packed, void *stream, void **handle) {
    int rc = validate(cfg);
    if (rc) return rc;
    HL_REQUIRE(names && ptrs && numels && packed && handle, "hl_unet_create: null argument");
    Net *n = new Net();
    n->cfg = *cfg;
    if (n->cfg.num_heads_upsample <= 0) n->cfg.num_heads_upsample = n->cfg.num_heads;
    for (int i = 0; i < n_tensors; ++i) n->sd[names[i]] = {static_cast<const float *>(ptrs[i]), numels[i]};
    n->dry = false;
    n->packed = static_cast<float *>(packed);
    n->st = (hipStream_t)stream;
    build(*n);
    if (!n->err.empty()) {
        rc = hl::fail(HL_ERR_INVALID, "hl_unet_create: %s", n->err.c_str());
        delete n;
        return rc;
    }
    if (n->cfg.controlnet) {
        // side stream + events of the two-tower overlap; any failure just leaves the overlap off (Exec::forward checks n.side)
        bool okc = hipStreamCreateWithFlags(&n->side, hipStreamNonBlocking) == hipSuccess;
        okc = okc && hipEventCreateWithFlags(&n->ev_fork, hipEventDisableTiming) == hipSuccess;
        okc = okc && hipEventCreateWithFlags(&n->ev_join, hipEventDisableTiming) == hipSuccess;
        n->ev_block.assign(n->in_blocks.size(), nullptr);
        for (auto &e : n->ev_block) okc = okc && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        if (!okc) {
            (void)hipGetLastError();
            if (n->side) { hipStreamDestroy(n->side); n->side = nullptr; }
        }
    }
    *handle = n;
    return HL_OK;
}

int hl_unet_set_overlap(void *handle, int enable) {
    HL_REQUIRE(handle, "hl_unet_set_overlap: null handle");
    static_cast<Net *>(handle)->overlap = enable != 0;
    return HL_OK;
}

int hl_unet_set_conv_mode(void *handle, int mode) {
    HL_REQUIRE(handle, "hl_unet_set_conv_mode: null handle");
    HL_REQUIRE(conv_mode_known(mode), "hl_unet_set_conv_mode: unknown mode %d", mode);
    static_cast<Net *>(handle)->conv_mode = mode;
    return HL_OK;
}

void hl_unet_destroy(void *handle) { delete static_cast<Net *>(handle); }

size_t hl_unet_workspace_bytes(void *handle, int B, int H, int W) {
    if (!handle || B <= 0) return 0;
    Net &n = *static_cast<Net *>(handle);
    Exec e(n, false, nullptr, nullptr, B, H, n.cfg.aware3d ? 3 * W : W);
    e.forward(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    WsLayout L;
    return ws_layout(e.off, e.act_need, e.stat_off, 0, &L) ? 0 : L.total;
}

int hl_unet_forward(void *handle, const float *x, const int64_t *t, const float *t_float, const float *x_cond,
                    const int64_t *y, float *out, int B, int H, int W, void *workspace, void *stream) {
    HL_REQUIRE(handle && x && (t || t_float) && out && workspace, "hl_unet_forward: null argument");
    Net &n = *static_cast<Net *>(handle);
    const int total_ds = 1 << (n.cfg.n_levels - 1);
    HL_REQUIRE(B >= 1 && B <= 16, "hl_unet_forward: batch %d outside [1,16]", B);
    HL_REQUIRE(H % total_ds == 0 && W % total_ds == 0, "hl_unet_forward: H,W must be divisible by %d", total_ds);
    HL_REQUIRE(!n.cfg.controlnet || x_cond, "hl_unet_forward: x_cond is required with cond_type='controlnet'");
    HL_REQUIRE(!(n.cfg.adagn || n.cfg.cross_attn) || (x_cond && H == 256 && W == 256),
               "hl_unet_forward: cond_type='AdaGN' / 'cross_attention' need x_cond and 256x256 inputs (Linear(64*64, ..))");
    HL_REQUIRE(n.cfg.num_classes == 0 || y, "hl_unet_forward: y is required for a class-conditional model");
    if (n.cfg.aware3d) W *= 3;                           // use_3d_aware: x is (B, 3*in_channels, H, W); the network runs on (B, in_channels, H, 3W)
    Exec dry(n, false, nullptr, nullptr, B, H, W);   // sizes only (host work, no launches)
    dry.forward(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    char *const ws = static_cast<char *>(workspace);
    WsLayout L;
    const int lrc = ws_layout(dry.off, dry.act_need, dry.stat_off, reinterpret_cast<uintptr_t>(ws), &L);
    if (lrc) return lrc;
    Exec e(n, true, ws, (hipStream_t)stream, B, H, W);
    e.act_need = dry.act_need;
    for (int i = 0; i < 2; ++i) e.lanes[i].act_ws = reinterpret_cast<float *>(ws + L.act_ws[i]);
    e.stat_base = ws + L.stats;
    e.stat_bytes = dry.stat_off;
    for (auto &row : n.census) for (auto &v : row) v = 0;
    e.forward(x, t, t_float, x_cond, y, out);
    return e.rc;
}

int hl_unet_dispatch_census(void *handle, int64_t *h_counts) {
    HL_REQUIRE(handle && h_counts, "hl_unet_dispatch_census: null argument");
    const Net &n = *static_cast<Net *>(handle);
    for (int p = 0; p < 4; ++p) for (int l = 0; l < 8; ++l) h_counts[p * 8 + l] = n.census[p][l];
    return HL_OK;
}

int hl_unet_dispatch_census_ex(void *handle, int64_t *h_counts, int rows) {
    HL_REQUIRE(handle && h_counts && rows >= 1 && rows <= 5, "hl_unet_dispatch_census_ex: bad argument");
    const Net &n = *static_cast<Net *>(handle);
    for (int p = 0; p < rows; ++p) for (int l = 0; l < 8; ++l) h_counts[p * 8 + l] = n.census[p][l];
    return HL_OK;
}

int hl_unet_profile(void *handle, int enable) {
    HL_REQUIRE(handle, "hl_unet_profile: null handle");
    Net &n = *static_cast<Net *>(handle);
    n.prof = enable != 0;
    n.spans.clear();
    n.ev_used = 0;
    return HL_OK;
}

int hl_unet_profile_read(void *handle, double *h_ms, double *h_flops, int64_t *h_launches) {
    return hl_unet_profile_read_ex(handle, h_ms, h_flops, nullptr, h_launches);
}

int hl_unet_profile_read_ex(void *handle, double *h_ms, double *h_flops, double *h_exec_flops, int64_t *h_launches) {
    HL_REQUIRE(handle && h_ms && h_flops && h_launches, "hl_unet_profile_read: null argument");
    Net &n = *static_cast<Net *>(handle);
    for (int i = 0; i < CAT_N; ++i) { h_ms[i] = 0; h_flops[i] = 0; h_launches[i] = 0; if (h_exec_flops) h_exec_flops[i] = 0; }
    if (n.spans.empty()) return HL_OK;
    HL_HIP(hipEventSynchronize(n.ev_pool[n.spans.back().b]));
    struct Agg { double ms = 0, fl = 0, ex = 0; long calls = 0; int key[5]; };
    std::vector<Agg> aggs;
    for (auto &sp : n.spans) {
        float ms = 0.f;
        HL_HIP(hipEventElapsedTime(&ms, n.ev_pool[sp.a], n.ev_pool[sp.b]));
        h_ms[sp.cat] += ms; h_flops[sp.cat] += sp.flops; h_launches[sp.cat] += 1;
        if (h_exec_flops) h_exec_flops[sp.cat] += sp.exec;
        if (sp.cat == CAT_CONV && sp.key[0] >= 0) {   // per convolution shape (kernel family, level, channels): which one dominates the step?
            Agg *hit = nullptr;
            for (auto &g : aggs) if (std::equal(g.key, g.key + 5, sp.key)) { hit = &g; break; }
            if (!hit) { aggs.emplace_back(); hit = &aggs.back(); std::copy(sp.key, sp.key + 5, hit->key); }
            float kms = ms;                                   // the kernel alone: from the event behind the GroupNorm pre-pass, if there was one
            if (sp.mid >= 0 && n.ev_pool[sp.mid]) HL_HIP(hipEventElapsedTime(&kms, n.ev_pool[sp.mid], n.ev_pool[sp.b]));
            hit->ms += kms; hit->fl += sp.flops; hit->ex += sp.exec; hit->calls += 1;
        }
    }
    n.dom[0] = n.dom[1] = n.dom[2] = n.dom[3] = 0;
    for (auto &g : aggs)
        if (g.ms > n.dom[0]) {
            n.dom[0] = g.ms; n.dom[1] = g.fl / g.calls; n.dom[2] = g.ex / g.calls; n.dom[3] = (double)g.calls;
            std::copy(g.key, g.key + 5, n.dom_key);
        }
    n.spans.clear();
    n.ev_used = 0;
    return HL_OK;
}

int hl_unet_profile_dominant(void *handle, double *h_vals, int *h_key) {
    HL_REQUIRE(handle && h_vals && h_key, "hl_unet_profile_dominant: null argument");
    const Net &n = *static_cast<Net *>(handle);
    for (int i = 0; i < 4; ++i) h_vals[i] = n.dom[i];
    for (int i = 0; i < 5; ++i) h_key[i] = n.dom_key[i];
    return HL_OK;
}

// ---- single ops for tests ------------------------------------------------------------------------
static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

static void conv_out_hw(int H, int W, int ks, int stride, int upsample, int *Ho, int *Wo) {
    const int pad = ks / 2, Hv = upsample ? 2 * H : H, Wv = upsample ? 2 * W : W;
    *Ho = (Hv + 2 * pad - ks) / stride + 1; *Wo = (Wv + 2 * pad - ks) / stride + 1;
}

// What plan_conv reads of a single-op layer: the geometry, the forms it may choose from and which rooms exist.  It asks only whether a
// pointer is there, so they all point at `at` (the queries have no buffer; conv2d_single puts the real ones in afterwards), and it plans
// with the conv_splitk_ws_bytes() every layer has inside hl_unet_forward.
static void single_conv_plan_args(ConvArgs &a, float *at, int mode, unsigned forms, int N, int H, int W, int Cin, int Cout, int ks, int stride,
                                  int upsample, bool with_gn, long out_pitch = 0) {
    a.in.N = N; a.in.H = H; a.in.W = W; a.in.C = Cin; a.in.pitch = Cin;
    a.Cout = Cout; a.ks = ks; a.stride = stride; a.ups = upsample; a.mode = mode;
    a.out.N = N; conv_out_hw(H, W, ks, stride, upsample, &a.out.H, &a.out.W); a.out.C = Cout; a.out.pitch = out_pitch ? out_pitch : Cout;
    for (int f = 0; f < hl::kWeightForms; ++f) a.w.p[f] = forms >> f & 1u ? at : nullptr;
    a.coefA = with_gn ? at : nullptr;
    a.act_ws = with_gn ? at : nullptr;
    a.act_ws_bytes = with_gn ? (size_t)N * H * W * Cin * sizeof(float) : 0;
    a.splitk_ws = at;
    a.splitk_ws_bytes = hl::conv_splitk_ws_bytes();
}
static size_t splitk_slab_bytes(const ConvArgs &a, const hl::ConvPlan &pl) {
    return pl.splits > 1 ? (size_t)pl.splits * a.out.N * a.out.H * a.out.W * a.Cout * sizeof(float) : 0;
}

// The scratch of one single-op convolution, stated once: the size queries and conv2d_single's carve both read it.  Byte offsets of the
// regions, each rounded to 256: the fp32 weight form at 0 | the largest other form the mode allows (only the one the plan reads is
// packed) | the materialised GroupNorm input (exactly when coefA is given) | per-image totals / abs-max of a raw fp16x2 input | the
// split-K slabs.  The plan is always made with the network's split-K room, so a single-op call takes the plan hl_unet_forward takes for
// the layer whatever the caller allocated; the region holds the slabs that plan writes (splits x M x Cout floats, the bound split_k
// itself cuts by), not the network's whole 64 MiB: the calls are made layer by layer with a fresh buffer each.  A GroupNorm in front can
// change the kernel family and with it the slabs, so a forward layer gets the larger of the two: with_gn adds the GroupNorm input, nothing else.
// Arguments no call accepts give a size of 0.
struct SingleConvRoom {
    size_t form, act, tot, splitk, total;
    unsigned forms;   // the forms the layer has under the mode
};
// The arguments of a single-op convolution, checked once for the call (conv2d_single), its two size queries and its two plan queries:
// null = the call accepts them, else what it refuses.  Beyond the ranges, conv2d's own refusals: a stride 2 behind the nearest-x2
// upsample, a GroupNorm in front of an upsample (nearest x2 + conv only ever follows a raw tensor) and a SiLU without a GroupNorm.
// A 1x1 convolution with stride 2 or behind an upsample is accepted: only k_conv / k_conv_dma / k_conv_bf3 take one (every other
// family asks for stride 1 and no upsample, or for ks 3), and those index the input by (oy * stride - pad, ox * stride - pad) or
// (y >> 1, x >> 1) with a bounds check per tap for any ks.
static const char *single_conv_refusal(int mode, int N, int H, int W, int Cin, int Cout, int ks, int stride, int upsample, bool with_gn, bool silu) {
    if (!conv_mode_known(mode)) return "unknown mode";
    if (N <= 0 || H <= 0 || W <= 0 || Cout <= 0) return "N, H, W and Cout must be positive";
    if (Cin <= 0 || Cin % 16) return "Cin must be a positive multiple of 16";
    if (ks != 1 && ks != 3) return "ks must be 1 or 3";
    if (stride != 1 && stride != 2) return "stride must be 1 or 2";
    if (stride == 2 && upsample) return "stride 2 behind an upsample";
    if (with_gn && upsample) return "a GroupNorm in front of an upsample";
    if (silu && !with_gn) return "SiLU without a GroupNorm";
    return nullptr;
}
static SingleConvRoom single_conv_room(int mode, int tf, int N, int H, int W, int Cin, int Cout, int ks, int stride, int upsample, bool with_gn) {
    SingleConvRoom r{};
    if (single_conv_refusal(mode, N, H, W, Cin, Cout, ks, stride, upsample, with_gn, false)) return r;
    r.forms = conv_forms(mode, true, tf != 0);
    size_t extra = 0;
    for (int f = 1; f < hl::kWeightForms; ++f) {
        const size_t b = r.forms >> f & 1u ? hl::conv_form_bytes((WeightForm)f, Cout, Cin, ks, false, upsample != 0) : 0;
        if (!b) r.forms &= ~(1u << f);   // (the layer has no such form)
        extra = std::max(extra, b);
    }
    r.form = up256(hl::conv_form_bytes(WeightForm::Fp32, Cout, Cin, ks));
    r.act = r.form + up256(extra);
    r.tot = r.act + (with_gn ? up256((size_t)N * H * W * Cin * sizeof(float)) : 0);
    r.splitk = r.tot + up256(hl::conv_stats_floats(N, (long)H * W) * sizeof(float));
    static float at;
    size_t slabs = 0;
    for (int gn = 0; gn <= (tf ? 0 : 1); ++gn) {      // (backward-data has no GroupNorm in front)
        ConvArgs a{};
        single_conv_plan_args(a, &at, mode, r.forms, N, H, W, Cin, Cout, ks, stride, upsample, gn != 0);
        slabs = std::max(slabs, splitk_slab_bytes(a, hl::plan_conv(a)));
    }
    r.total = r.splitk + up256(slabs);
    return r;
}

// One convolution through the kernels of the network.  Cin = channels of `in` (multiple of 16); the weight tensor covers
// Cin_w <= Cin of them (the rest are zero-padded channels with zero weights).  tf = 1: `w` is laid out (Cin_w, Cout, ks, ks) and is
// read flipped and channel-transposed - the backward-data convolution of the training path.  Only the weight layout the chosen
// kernel reads is packed (plan_conv decides first).
static int g_single_op_scale_from_totals = 0;   // hl_debug_set_single_op_scale_source (test switch)
static int conv2d_single(int mode, const float *in, int N, int H, int W, int Cin, const float *w_oihw, const float *bias, int Cout,
                         int ks, int stride, int upsample, const float *coefA, const float *coefB, int silu,
                         const float *residual, float *out, void *scratch, size_t scratch_bytes, void *stream,
                         float *stats = nullptr, int *stat_slots = nullptr, int tf = 0, int Cin_w = -1, long out_pitch = 0) {
    const char *refused = single_conv_refusal(mode, N, H, W, Cin, Cout, ks, stride, upsample, coefA != nullptr, silu != 0);
    HL_REQUIRE(!refused, "hl_conv2d_nhwc: %s (mode %d, N %d, H %d, W %d, Cin %d, Cout %d, ks %d, stride %d, upsample %d)", refused, mode, N, H, W, Cin, Cout,
               ks, stride, upsample);
    if (Cin_w < 0) Cin_w = Cin;
    HL_REQUIRE(Cin_w <= Cin, "hl_conv2d_nhwc: the weight has more input channels than the tensor");
    hipStream_t st = (hipStream_t)stream;
    const SingleConvRoom room = single_conv_room(mode, tf, N, H, W, Cin, Cout, ks, stride, upsample, coefA != nullptr);
    HL_REQUIRE(room.total, "hl_conv2d_nhwc: bad argument (mode %d, N %d, H %d, W %d, Cin %d, Cout %d, ks %d, stride %d)", mode, N, H, W, Cin, Cout, ks, stride);
    HL_REQUIRE(scratch && scratch_bytes >= room.total, "hl_conv2d_nhwc: scratch too small (%zu bytes, hl_conv2d_scratch_bytes says %zu)",
               scratch_bytes, room.total);
    char *sc = static_cast<char *>(scratch);
    void *extra_dst = sc + room.form;
    ConvArgs a{};
    single_conv_plan_args(a, static_cast<float *>(scratch), mode, room.forms, N, H, W, Cin, Cout, ks, stride, upsample, coefA != nullptr, out_pitch);
    // every form the layer has under the mode points at that room, for plan_conv to choose from
    for (int f = 1; f < hl::kWeightForms; ++f) if (a.w.p[f]) a.w.p[f] = extra_dst;
    if (coefA) a.act_ws = reinterpret_cast<float *>(sc + room.act);      // the materialised GroupNorm input (DMA path)
    a.splitk_ws = reinterpret_cast<float *>(sc + room.splitk);
    a.in.p = const_cast<float *>(in); a.bias = bias;
    a.coefA = coefA; a.coefB = coefB; a.act = silu;
    a.out.p = out;
    a.res = residual; a.res_pitch = Cout;
    float *tot_room = reinterpret_cast<float *>(sc + room.tot);
    a.stats = stats;
    if (stats) HL_HIP(hipMemsetAsync(stats, 0, hl::conv_stats_floats(N, (long)a.out.H * a.out.W) * sizeof(float), st));   // the epilogues ADD to the totals
    const hl::ConvPlan pl = hl::plan_conv(a);
    // (no tensor changes a split; a test switch of the dispatch flipped between the query and the call can: refused, never an overrun)
    HL_REQUIRE(room.splitk + splitk_slab_bytes(a, pl) <= room.total, "hl_conv2d_nhwc: the plan splits K further than hl_conv2d_scratch_bytes planned");
    // the room holds that form only: no kernel argument points at the others
    const WeightForm form = pl.form;
    a.w = a.w.only(hl::form_bit(WeightForm::Fp32) | hl::form_bit(form));
    int rc = hl::conv_pack_form(form, w_oihw, Cout, Cin_w, Cin, ks, form == WeightForm::Fp32 ? scratch : extra_dst, st, tf, mode == HL_CONV_FP16);
    if (rc) return rc;
    if (pl.path == hl::ConvPath::Fp16x2 && !coefA) {   // fp16x2 products on a raw input: the largest |x| of every image fixes the power-of-two scale of the activation planes
        // (in the network the producers' sum x^2 bounds it; here one pass over the tensor - exact at any magnitude, which the backward-data calls need: gradients are 1e-4 ... 1e-9)
        if (g_single_op_scale_from_totals) {      // (test switch: the network's scale source - the group totals - on a single layer)
            rc = hl::tensor_totals(a.in, tot_room, st);
            if (rc) return rc;
            a.in_stats = tot_room;
        } else {
            rc = hl::tensor_absmax(a.in, tot_room, st);
            if (rc) return rc;
            a.in_absmax = tot_room;
        }
    }
    if (stat_slots) *stat_slots = pl.stat_slots;
    return hl::conv2d(a, pl, st);
}

size_t hl_conv2d_scratch_bytes(int conv_mode, int N, int H, int W, int Cin, int Cout, int ks, int stride, int upsample, int with_gn) {
    return single_conv_room(conv_mode, 0, N, H, W, Cin, Cout, ks, stride, upsample, with_gn != 0).total;
}

// The plan conv2d_single makes for the same arguments, without a buffer (the plan queries; host arithmetic: no HIP call).  silu and
// with_stats: what the call puts into ConvArgs::act and ::stats before it plans (hl_conv2d_nhwc_gn wants the statistics).  false:
// arguments no call accepts.
static bool single_conv_query_plan(int mode, int tf, int N, int H, int W, int Cin, int Cout, int ks, int stride, int upsample, bool with_gn,
                                   long out_pitch, hl::ConvPlan *pl, bool silu = false, bool with_stats = false) {
    if (single_conv_refusal(mode, N, H, W, Cin, Cout, ks, stride, upsample, with_gn, silu)) return false;
    const SingleConvRoom room = single_conv_room(mode, tf, N, H, W, Cin, Cout, ks, stride, upsample, with_gn);
    if (!room.total) return false;
    static float at;
    ConvArgs a{};
    single_conv_plan_args(a, &at, mode, room.forms, N, H, W, Cin, Cout, ks, stride, upsample, with_gn, out_pitch);
    a.act = silu;
    a.stats = with_stats ? &at : nullptr;
    *pl = hl::plan_conv(a);
    return true;
}

int hl_conv2d_plan(int conv_mode, int N, int H, int W, int Cin, int Cout, int ks, int stride, int upsample, int with_gn, int *h_kernel, int *h_splits) {
    HL_REQUIRE(h_kernel && h_splits, "hl_conv2d_plan: null argument");
    hl::ConvPlan pl;
    HL_REQUIRE(single_conv_query_plan(conv_mode, 0, N, H, W, Cin, Cout, ks, stride, upsample, with_gn != 0, 0, &pl),
               "hl_conv2d_plan: bad argument (mode %d, N %d, H %d, W %d, Cin %d, Cout %d, ks %d, stride %d, upsample %d, with_gn %d)", conv_mode, N, H, W, Cin,
               Cout, ks, stride, upsample, with_gn);
    *h_kernel = (int)pl.kernel; *h_splits = pl.splits;
    return HL_OK;
}

static_assert((int)hl::ConvPrePass::None == HL_PRE_NONE && (int)hl::ConvPrePass::Dense == HL_PRE_DENSE && (int)hl::ConvPrePass::Blocked == HL_PRE_BLOCKED &&
                  (int)hl::ConvPrePass::Half == HL_PRE_HALF && (int)hl::ConvPrePass::TwoPlane == HL_PRE_TWO_PLANE,
              "humanliff_hip.h documents ConvPrePass's numbers");
static_assert((int)hl::ConvStatsBy::None == HL_STATS_BY_NONE && (int)hl::ConvStatsBy::Epilogue == HL_STATS_BY_EPILOGUE &&
                  (int)hl::ConvStatsBy::Finish == HL_STATS_BY_FINISH,
              "humanliff_hip.h documents ConvStatsBy's numbers");
int hl_conv2d_plan_ex(int conv_mode, int N, int H, int W, int Cin, int Cout, int ks, int stride, int upsample, int with_gn, int silu, int with_stats,
                      int *h_plan) {
    HL_REQUIRE(h_plan, "hl_conv2d_plan_ex: null argument");
    hl::ConvPlan pl;
    HL_REQUIRE(single_conv_query_plan(conv_mode, 0, N, H, W, Cin, Cout, ks, stride, upsample, with_gn != 0, 0, &pl, silu != 0, with_stats != 0),
               "hl_conv2d_plan_ex: bad argument (mode %d, N %d, H %d, W %d, Cin %d, Cout %d, ks %d, stride %d, upsample %d, with_gn %d, silu %d)", conv_mode, N,
               H, W, Cin, Cout, ks, stride, upsample, with_gn, silu);
    h_plan[HL_PLAN_KERNEL] = (int)pl.kernel; h_plan[HL_PLAN_SPLITS] = pl.splits; h_plan[HL_PLAN_CFG] = pl.cfg; h_plan[HL_PLAN_TILE8] = pl.tile8 ? 1 : 0;
    h_plan[HL_PLAN_GN_MODE] = pl.gn_mode; h_plan[HL_PLAN_PRE] = (int)pl.pre; h_plan[HL_PLAN_STATS_BY] = (int)pl.stats_by;
    h_plan[HL_PLAN_STAT_SLOTS] = pl.stat_slots; h_plan[HL_PLAN_KT_PER] = pl.kt_per;
    return HL_OK;
}

// What hl_conv2d_nhwc_gn puts in front: the totals of the output and the scratch of a GroupNorm pass over it.
struct GnPrefix { size_t gn, conv; };   // byte offsets of the GroupNorm scratch and of the convolution's room (the totals sit at 0)
static GnPrefix conv_gn_prefix(int N, int H, int W, int ks, int stride, int upsample) {
    int Ho, Wo;
    conv_out_hw(H, W, ks, stride, upsample, &Ho, &Wo);
    GnPrefix p;
    p.gn = up256(hl::conv_stats_floats(N, (long)Ho * Wo) * sizeof(float));
    p.conv = p.gn + up256(hl::gn_scratch_floats(N) * sizeof(float));
    return p;
}

size_t hl_conv2d_gn_scratch_bytes(int conv_mode, int N, int H, int W, int Cin, int Cout, int ks, int stride, int upsample, int with_gn) {
    const size_t conv = hl_conv2d_scratch_bytes(conv_mode, N, H, W, Cin, Cout, ks, stride, upsample, with_gn);
    return conv ? conv_gn_prefix(N, H, W, ks, stride, upsample).conv + conv : 0;
}

// What hl_conv2d_nhwc_bwd_data puts in front: the zero-stuffed (stride 2) or upsampled (nearest x2) gradient.
static size_t bwd_data_prefix(int N, int Ho, int Wo, int Cy, int stride, int upsample, int Cx) {
    return stride == 2 ? up256((size_t)N * 4 * Ho * Wo * Cy * sizeof(float)) : upsample ? up256((size_t)N * Ho * Wo * Cx * sizeof(float)) : 0;
}

// The forward convolution a backward-data call runs (tf = 1), stated once for the call, its scratch query and its plan query: on the
// (H, W) grid - the zero-stuffed (2Ho, 2Wo) one for stride 2 - from the Cy channels of the gradient to the Cin input channels of the
// layer, stride 1, nothing in front, stored with a pitch of Cx.  what: the refusal (null = the arguments are fine).
struct BwdDataConv { int H, W; const char *what; };
static BwdDataConv bwd_data_conv(int conv_mode, int Ho, int Wo, int Cy, int Cout, int Cin, int ks, int stride, int upsample, int Cx) {
    BwdDataConv c{};
    const int s = stride == 2 ? 2 : 1;
    c.H = s * Ho; c.W = s * Wo;
    if (!(conv_mode_known(conv_mode) && conv_mode != HL_CONV_BF16X3 && conv_mode != HL_CONV_FP32_MFMA)) c.what = "mode";   // (the training path's modes)
    else if (!(Cy % 16 == 0 && Cout <= Cy && Cin <= Cx && (ks == 1 || ks == 3) && (stride == 1 || (stride == 2 && !upsample && ks == 3)) &&
               (!upsample || (Cx % 4 == 0 && Ho % 2 == 0 && Wo % 2 == 0)) && Cx > 0))      // (an upsampled image has even sides)
        c.what = "bad argument";
    return c;
}

size_t hl_conv2d_bwd_data_scratch_bytes(int conv_mode, int N, int Ho, int Wo, int Cy, int Cout, int Cin, int ks, int stride, int upsample, int Cx) {
    const BwdDataConv c = bwd_data_conv(conv_mode, Ho, Wo, Cy, Cout, Cin, ks, stride, upsample, Cx);   // (Cout: the weight's output channels - the convolution reads all Cy of the gradient)
    const size_t conv = c.what ? 0 : single_conv_room(conv_mode, 1, N, c.H, c.W, Cy, Cin, ks, 1, 0, false).total;
    return conv ? bwd_data_prefix(N, Ho, Wo, Cy, stride, upsample, Cx) + conv : 0;
}

int hl_conv2d_bwd_data_plan(int conv_mode, int N, int Ho, int Wo, int Cy, int Cout, int Cin, int ks, int stride, int upsample, int Cx,
                            int *h_kernel, int *h_splits) {
    HL_REQUIRE(h_kernel && h_splits, "hl_conv2d_bwd_data_plan: null argument");
    const BwdDataConv c = bwd_data_conv(conv_mode, Ho, Wo, Cy, Cout, Cin, ks, stride, upsample, Cx);
    HL_REQUIRE(!c.what, "hl_conv2d_bwd_data_plan: %s (mode %d)", c.what, conv_mode);
    hl::ConvPlan pl;
    HL_REQUIRE(single_conv_query_plan(conv_mode, 1, N, c.H, c.W, Cy, Cin, ks, 1, 0, false, Cx, &pl), "hl_conv2d_bwd_data_plan: bad argument");
    *h_kernel = (int)pl.kernel; *h_splits = pl.splits;
    return HL_OK;
}

int hl_conv2d_nhwc_bwd_data(int conv_mode, const float *dy, int N, int Ho, int Wo, int Cy, const float *w_oihw, int Cout, int Cin, int ks,
                            int stride, int upsample, float *dx, int Cx, void *scratch, size_t scratch_bytes, void *stream) {
    const BwdDataConv c = bwd_data_conv(conv_mode, Ho, Wo, Cy, Cout, Cin, ks, stride, upsample, Cx);
    HL_REQUIRE(!c.what, "hl_conv2d_nhwc_bwd_data: %s (mode %d)", c.what, conv_mode);
    HL_REQUIRE(dy && w_oihw && dx && scratch, "hl_conv2d_nhwc_bwd_data: null argument");
    const size_t need = hl_conv2d_bwd_data_scratch_bytes(conv_mode, N, Ho, Wo, Cy, Cout, Cin, ks, stride, upsample, Cx);
    HL_REQUIRE(need, "hl_conv2d_nhwc_bwd_data: bad argument");
    HL_REQUIRE(scratch_bytes >= need, "hl_conv2d_nhwc_bwd_data: scratch too small (%zu bytes, hl_conv2d_bwd_data_scratch_bytes says %zu)",
               scratch_bytes, need);
    // d input = convolution of d output with W'[ci][co][ky][kx] = W[co][ci][ks-1-ky][ks-1-kx]  (packed straight from w, tf = 1);
    // stride 2: on the zero-stuffed gradient; nearest-x2 upsample in front of the conv: the 2x2 blocks of the result are summed
    hipStream_t st = (hipStream_t)stream;
    char *sc = static_cast<char *>(scratch);
    const size_t pre = bwd_data_prefix(N, Ho, Wo, Cy, stride, upsample, Cx);
    const float *in = dy;
    float *out = dx;
    int rc;
    if (stride == 2) {
        float *z = reinterpret_cast<float *>(sc);
        rc = hl_zero_stuff2_nhwc(dy, N, Ho, Wo, Cy, z, stream);
        if (rc) return rc;
        in = z;
    }
    if (upsample) {      // dy lives on the (2H, 2W) grid = (Ho, Wo); dx on (Ho/2, Wo/2)
        out = reinterpret_cast<float *>(sc);
        if (Cx != Cin) HL_HIP(hipMemsetAsync(out, 0, pre, st));
    }
    rc = conv2d_single(conv_mode, in, N, c.H, c.W, Cy, w_oihw, nullptr, Cin, ks, 1, 0, nullptr, nullptr, 0, nullptr, out, sc + pre, scratch_bytes - pre,
                       stream, nullptr, nullptr, 1, Cout, Cx);
    if (rc || !upsample) return rc;
    return hl_upsample2_backward_nhwc(out, N, Ho / 2, Wo / 2, Cx, dx, stream);
}

int hl_conv2d_nhwc_gn(int conv_mode, const float *in, int N, int H, int W, int Cin, const float *w_oihw, const float *bias, int Cout,
                      int ks, int stride, int upsample, const float *coefA, const float *coefB, int silu, const float *residual,
                      float *out, const float *gamma, const float *beta, float *next_coefA, float *next_coefB, int *h_used_stats,
                      void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(conv_mode_known(conv_mode), "hl_conv2d_nhwc_gn: unknown mode %d", conv_mode);
    HL_REQUIRE(gamma && beta && next_coefA && next_coefB && scratch, "hl_conv2d_nhwc_gn: null argument");
    const size_t need = hl_conv2d_gn_scratch_bytes(conv_mode, N, H, W, Cin, Cout, ks, stride, upsample, coefA != nullptr);
    HL_REQUIRE(need, "hl_conv2d_nhwc_gn: bad argument");
    HL_REQUIRE(scratch_bytes >= need, "hl_conv2d_nhwc_gn: scratch too small (%zu bytes, hl_conv2d_gn_scratch_bytes says %zu)", scratch_bytes, need);
    const GnPrefix pre = conv_gn_prefix(N, H, W, ks, stride, upsample);
    float *stats = static_cast<float *>(scratch);
    float *gn_scr = reinterpret_cast<float *>(static_cast<char *>(scratch) + pre.gn);
    int slots = 0;
    int rc = conv2d_single(conv_mode, in, N, H, W, Cin, w_oihw, bias, Cout, ks, stride, upsample, coefA, coefB, silu, residual, out,
                           static_cast<char *>(scratch) + pre.conv, scratch_bytes - pre.conv, stream, stats, &slots);
    if (rc) return rc;
    View v; v.p = out; v.N = N; conv_out_hw(H, W, ks, stride, upsample, &v.H, &v.W); v.C = Cout; v.pitch = Cout;
    if (h_used_stats) *h_used_stats = slots;
    if (slots > 0) {
        return hl::groupnorm_coef_stats(v, stats, gamma, beta, nullptr, 0, next_coefA, next_coefB, (hipStream_t)stream);
    }
    return hl::groupnorm_coef(v, gamma, beta, nullptr, 0, next_coefA, next_coefB, gn_scr, (hipStream_t)stream);
}

int hl_conv2d_nhwc(const float *in, int N, int H, int W, int Cin, const float *w_oihw, const float *bias, int Cout, int ks,
                   int stride, int upsample, const float *coefA, const float *coefB, int silu, const float *residual,
                   float *out, void *scratch, size_t scratch_bytes, void *stream) {
    // (plain entry point: direct convolution only; hl_conv2d_nhwc_mode(HL_CONV_FP32, ...) adds the Winograd copy)
    return conv2d_single(HL_CONV_FP32_DIRECT, in, N, H, W, Cin, w_oihw, bias, Cout, ks, stride, upsample, coefA, coefB, silu, residual, out,
                         scratch, scratch_bytes, stream);
}

int hl_conv2d_nhwc_mode(int conv_mode, const float *in, int N, int H, int W, int Cin, const float *w_oihw, const float *bias,
                        int Cout, int ks, int stride, int upsample, const float *coefA, const float *coefB, int silu,
                        const float *residual, float *out, void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(conv_mode_known(conv_mode), "hl_conv2d_nhwc_mode: unknown mode %d", conv_mode);
    return conv2d_single(conv_mode, in, N, H, W, Cin, w_oihw, bias, Cout, ks, stride, upsample, coefA, coefB, silu, residual, out,
                         scratch, scratch_bytes, stream);
}

int hl_debug_set_h16_min_blocks(long v) { hl::set_h16_min_blocks(v); return HL_OK; }
int hl_debug_set_single_op_scale_source(int from_totals) { g_single_op_scale_from_totals = from_totals != 0; return HL_OK; }
int hl_debug_set_attention_tiling(int query_tiles, int placement) { return hl::debug_set_attention_tiling(query_tiles, placement); }

size_t hl_groupnorm_scratch_bytes(int N) { return hl::gn_scratch_floats(N) * sizeof(float); }

int hl_groupnorm_coef(const float *x, int N, int H, int W, int C, const float *gamma, const float *beta, const float *emb,
                      float *coefA, float *coefB, void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(scratch && scratch_bytes >= hl_groupnorm_scratch_bytes(N), "hl_groupnorm_coef: scratch too small (%zu bytes, hl_groupnorm_scratch_bytes says %zu)",
               scratch_bytes, hl_groupnorm_scratch_bytes(N));
    View v; v.p = const_cast<float *>(x); v.N = N; v.H = H; v.W = W; v.C = C; v.pitch = C;
    return hl::groupnorm_coef(v, gamma, beta, emb, 2L * C, coefA, coefB, static_cast<float *>(scratch), (hipStream_t)stream);
}

int hl_timestep_embedding(const int64_t *t, const float *t_float, int B, int dim, float *out, void *stream) {
    HL_REQUIRE(dim % 2 == 0, "hl_timestep_embedding: odd dim %d", dim);
    return hl::timestep_embedding(t, t_float, B, dim, out, (hipStream_t)stream);
}

int hl_attention_nhwc(const float *qkv, int N, int T, int C, int heads, float *out, void *stream) {
    return hl::attention(qkv, N, T, C, heads, out, (hipStream_t)stream);
}

int hl_attention_nhwc_mode(int conv_mode, const float *qkv, int N, int T, int C, int heads, float *out, void *stream) {
    return hl::attention(qkv, N, T, C, heads, out, (hipStream_t)stream, conv_mode == HL_CONV_FP32);
}

size_t hl_attention_backward_scratch_bytes(int N, int T, int C, int heads) { return hl::attention_backward_scratch_bytes(N, T, C, heads); }

int hl_attention_nhwc_backward(const float *qkv, const float *out, const float *dout, int N, int T, int C, int heads, float *dqkv,
                               void *scratch, size_t scratch_bytes, void *stream) {
    return hl::attention_backward(qkv, out, dout, N, T, C, heads, dqkv, scratch, scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
