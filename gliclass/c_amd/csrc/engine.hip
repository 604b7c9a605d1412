// Engine = what g_ort->CreateSession + g_ort->Run are to /root/reference/src/model.c:173,269:
// weight residency in HBM, workspace management, and the per-forward launch sequence on ONE HIP
// stream.  Implements include/gliclass_hip.h.  No CPU fallback exists: without a GPU every entry
// point fails loudly through glc_last_error().  The developer entries that allocate buffers of their
// own or launch kernels outside a forward (microbenchmarks, glc_debug_gemm_run, workspace read-back)
// are in engine_debug.hip.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "engine_internal.h"
#include "glc_layout.h"

namespace {
thread_local std::string g_err;
}
void glc_set_err(const std::string& s) { g_err = s; }

namespace {

constexpr int kActScLow = -5;
// the launchers' view of the engine for one forward (glc_kernels.h): fp8 guard counter and activation exponent, reset behind it
struct GxScope {
    explicit GxScope(glc_engine* e) { glc_gx_sat_ptr() = e->d_gxsat; glc_gx_act_sc() = e->act_sc; }
    ~GxScope() { glc_gx_sat_ptr() = nullptr; glc_gx_act_sc() = 0; }
};

// Captured-graph replay: drop every cached graph and every remembered key (the stream may still be running one of them)
void graph_clear(glc_engine* e) {
    if (e->graphs.empty() || e->capturing) return;
    bool any = false;
    for (const GraphEntry& g : e->graphs) any = any || g.exec;
    if (any) { (void)hipSetDevice(e->device); (void)hipStreamSynchronize(e->stream); }
    for (GraphEntry& g : e->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    e->graphs.clear();
}

void* dmalloc(glc_engine* e, size_t bytes, bool zero = true) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    if (e->capturing) { glc_set_err("allocation inside a captured forward"); return nullptr; }      // (graph_forward then runs this forward eagerly)
    if (hipMalloc(&p, bytes) != hipSuccess) { glc_set_err("hipMalloc failed for " + std::to_string(bytes) + " bytes"); return nullptr; }
    if (zero && hipMemsetAsync(p, 0, bytes, e->stream) != hipSuccess) { glc_set_err("hipMemset failed"); return nullptr; }
    e->allocs.push_back(p);
    return p;
}
void dfree(glc_engine* e, void* p) {
    if (!p || e->capturing) return;        // (capturing: the buffer stays in allocs; the allocation that follows refuses)
    // A cached graph may hold this address.  Deliberately conservative: EVERY freed engine buffer bumps the generation and drops the cache
    // (with graphs cached that is a stream synchronise), also one no graph can name — a load-time temporary, the hidden dump.  Frees happen
    // at load, when the workspace grows and on the first forward of a pipeline, never in steady state, and tracking which buffers a
    // graph names would buy nothing there.
    ++e->ws_gen; graph_clear(e);
    for (size_t i = 0; i < e->allocs.size(); ++i)
        if (e->allocs[i] == p) { e->allocs[i] = e->allocs.back(); e->allocs.pop_back(); break; }
    (void)hipFree(p);
}

struct Prof {
    glc_engine* e; int idx = -1;
    Prof(glc_engine* e_, int cls) : e(e_) {
        if (!e->profile) return;
        if (e->ev_used == e->evs.size()) {
            glc_engine::Ev v{};
            if (hipEventCreate(&v.a) != hipSuccess || hipEventCreate(&v.b) != hipSuccess) return;
            e->evs.push_back(v);
        }
        idx = (int)e->ev_used++;
        e->evs[idx].cls = cls;
        (void)hipEventRecord(e->evs[idx].a, e->stream);
    }
    ~Prof() { if (idx >= 0) (void)hipEventRecord(e->evs[idx].b, e->stream); }
};

void prof_collect(glc_engine* e) {
    for (size_t i = 0; i < e->ev_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e->evs[i].a, e->evs[i].b) == hipSuccess) { e->prof_ms[e->evs[i].cls] += ms; e->prof_n[e->evs[i].cls]++; }
    }
    e->ev_used = 0;
}

// host f32 -> device f32
float* upload_f32(glc_engine* e, const float* src, size_t n) {
    float* d = (float*)dmalloc(e, n * sizeof(float), false);
    if (!d) return nullptr;
    if (hipMemcpyAsync(d, src, n * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess) { glc_set_err("H2D failed"); return nullptr; }
    return d;
}
// host f32 -> device T at dst (dst preallocated), via a temporary f32 staging buffer
bool upload_as(glc_engine* e, const float* src, size_t n, void* dst, float* staging) {
    if (hipMemcpyAsync(staging, src, n * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess) { glc_set_err("H2D failed"); return false; }
    const char* m = glc_launch_convert(e->stream, e->dtype, staging, dst, n);
    if (m) { glc_set_err(m); return false; }
    return hipStreamSynchronize(e->stream) == hipSuccess;   // staging is reused by the caller
}

constexpr int kFp8Sticky = 2;
bool init_range_guard(glc_engine* e) {
    if (e->d_gxsat) return true;
    e->d_gxsat = (unsigned*)dmalloc(e, 2 * sizeof(unsigned), false);
    if (!e->d_gxsat || hipMemset(e->d_gxsat, 0, 2 * sizeof(unsigned)) != hipSuccess) { glc_set_err("range-guard counter alloc failed"); return false; }
    if (hipHostMalloc((void**)&e->h_gxsat, 2 * sizeof(unsigned), hipHostMallocDefault) != hipSuccess) { e->h_gxsat = nullptr; glc_set_err("range-guard host slot alloc failed"); return false; }
    e->h_gxsat[0] = e->h_gxsat[1] = 0;
    return true;
}
// free a workspace buffer and allocate it again (zeroed) at its new size
template <class T> bool regrow(glc_engine* e, T*& p, size_t bytes) {
    dfree(e, p);
    p = (T*)dmalloc(e, bytes);
    return p != nullptr;
}
// a host table in device memory (hipMemcpy: complete on return)
template <class T> T* upload_table(glc_engine* e, const std::vector<T>& t, const char* what) {
    T* d = (T*)dmalloc(e, t.size() * sizeof(T), false);
    if (!d) return nullptr;
    if (hipMemcpy(d, t.data(), t.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { glc_set_err(std::string(what) + " upload failed"); return nullptr; }
    return d;
}

// decoder / ModernBERT: one cos / sin table per (Sp, theta); ModernBERT's global and local layers use two bases
bool build_rope_tables(glc_engine* e, int Sp) {
    const glc_model_config& c = e->cfg;
    if (c.backbone == GLC_BACKBONE_BERT || c.backbone == GLC_BACKBONE_T5) {
        // no rotation on these backbones: the layout passes get a table of cos = 1, sin = 0 (x 1 - y 0 = x, exact), filed under base 0
        if (e->ropes.count({Sp, 0.f})) return true;
        std::vector<float> t((size_t)Sp * (c.head_dim / 2) * 2);
        for (size_t i = 0; i < t.size(); i += 2) { t[i] = 1.f; t[i + 1] = 0.f; }
        float* d = upload_table(e, t, "identity rotation table");
        if (!d) return false;
        e->ropes[{Sp, 0.f}] = d;
        return true;
    }
    const float thetas[2] = {c.rope_theta, c.backbone == GLC_BACKBONE_MODERNBERT ? c.rope_theta_local : c.rope_theta};
    for (float theta : thetas) {
        if (e->ropes.count({Sp, theta})) continue;
        // Q2:86 inv_freq = 1 / base^(arange(0,d,2)/d) in float32; Q2:97-100 freqs = inv_freq * position, then cos / sin
        const int hd2 = c.head_dim / 2;
        std::vector<float> t((size_t)Sp * hd2 * 2);
        for (int s = 0; s < Sp; ++s)
            for (int i = 0; i < hd2; ++i) {
                const float inv = 1.0f / powf(theta, (float)(2 * i) / (float)c.head_dim);
                const float f = inv * (float)s;
                t[((size_t)s * hd2 + i) * 2] = cosf(f);
                t[((size_t)s * hd2 + i) * 2 + 1] = sinf(f);
            }
        float* d = upload_table(e, t, "rope table");
        if (!d) return false;
        e->ropes[{Sp, theta}] = d;
    }
    return true;
}

// T5: the relative-position bias of one padded length, rpb [t5_heads][2 Sp] fp32 in the log2 units of the exp2 softmax:
// rel_bias[bucket(delta), h] log2(e) at entry delta + Sp - 1, delta = key - query (T5:264-281 compute_bias; the last entry of a head is never read)
bool build_rpb_table(glc_engine* e, int Sp) {
    if (e->rpbs.count(Sp)) return true;
    const glc_model_config& c = e->cfg;
    std::vector<int32_t> bk(2 * Sp - 1);
    glc_t5_bucket_table(Sp, c.rel_buckets, c.rel_max_distance, bk.data());
    std::vector<float> t((size_t)e->t5_heads * 2 * Sp, 0.f);
    for (int h = 0; h < c.heads; ++h)
        for (int j = 0; j < 2 * Sp - 1; ++j) t[(size_t)h * 2 * Sp + j] = e->rel_bias[(size_t)bk[j] * c.heads + h] * 1.4426950408889634f;
    float* d = upload_table(e, t, "relative-position bias table");
    if (!d) return false;
    e->rpbs[Sp] = d;
    return true;
}

// DeBERTa: the relative-position tables of one padded length.  dtabs[Sp] guards the whole block, so it is written last: a call that
// fails part-way leaves no entry and the next forward at this length builds every table again.
bool build_position_tables(glc_engine* e, int Sp) {
    if (e->dtabs.count(Sp)) return true;
    const glc_model_config& c = e->cfg;
    const size_t es = esize(e->dtype);
    std::vector<int32_t> t(2 * Sp - 1);
    glc_delta_table(Sp, c.pos_buckets, c.max_rel_pos, t.data());
    int32_t* d = upload_table(e, t, "dtab");
    if (!d) return false;
    auto dl_of = [&](long long j) { const long long r = j - 64; return t[r < 0 ? 0 : (r > (long long)t.size() - 1 ? t.size() - 1 : (size_t)r)]; };
    // band-kernel addressing table: entry j <-> relative distance clamp(j - 64, 0, 2Sp-2) - (Sp-1); x = byte offset of PQ row
    // delta in the Q fragment layout, y = byte offset of PK row delta in the K layout (pi on the row) — glc_layout.h
    std::vector<int2> o(t.size() + 128);
    for (size_t j = 0; j < o.size(); ++j) {
        const int dl = dl_of((long long)j);
        o[j].x = ((dl >> 5) * 2048 + (dl & 31) * 8) * (int)es;
        o[j].y = ((dl >> 5) * 2048 + glc_pi32(dl & 31) * 8) * (int)es;
    }
    int2* od = upload_table(e, o, "otab");
    if (!od) return false;
    e->otabs[Sp] = od;
    if (es == 4) {
        // MX band kernel (attention_mx.hip, round 6): the same rows as ready-made load offsets into the PLANAR tile images of the position tables
        // (glc_layout.h) — per lane half hh and entry j (NE = 2 Sp + 512 entries: 64 clamped ones in front, the rest behind, so that no index the
        // kernel forms needs a clamp): .x = offset of the PQ row of entry j, .y = offset of the PK row of entry NE - 1 - j (the PK half runs
        // BACKWARDS: a lane that adds its column c to a wave-uniform base walks the PQ rows up and the PK rows down with the same per-lane
        // register); offset = tile * 8192 + slot * 16 + hh * 512: the lane's 16 bytes of f16 unit 0; unit s at + s * 1024, MX plane k at + 4096 + k * 1024
        const int NE = 2 * Sp + 512;
        std::vector<int2> m((size_t)2 * NE);
        for (int hh = 0; hh < 2; ++hh)
            for (int j = 0; j < NE; ++j) {
                const int dq = dl_of(j), dk = dl_of(NE - 1 - j);
                m[(size_t)hh * NE + j] = make_int2((dq >> 5) * 8192 + (dq & 31) * 16 + hh * 512, (dk >> 5) * 8192 + glc_pi32(dk & 31) * 16 + hh * 512);
            }
        int2* md = upload_table(e, m, "mtab");
        if (!md) return false;
        e->mtabs[Sp] = md;
    }
    // saturation points of the table: delta == P-1 for every q-k >= rsat_pos, delta == 0 for every q-k <= rsat_neg
    int rp = Sp, rn = -Sp;
    for (int r = Sp - 1; r >= -(Sp - 1) && t[r + Sp - 1] == 2 * (c.pos_buckets > 0 ? c.pos_buckets : c.max_rel_pos) - 1; --r) rp = r;
    for (int r = -(Sp - 1); r <= Sp - 1 && t[r + Sp - 1] == 0; ++r) rn = r;
    e->dsat[Sp] = std::make_pair(rp, rn);
    e->dtabs[Sp] = d;
    return true;
}

bool ensure_capacity(glc_engine* e, int B, int S, int C) {
    const glc_model_config& c = e->cfg;
    if (!init_range_guard(e)) return false;
    if (!e->splitk_ws) {
        e->splitk_ws_bytes = (size_t)64 << 20;
        e->splitk_ws = (float*)dmalloc(e, e->splitk_ws_bytes, false);
        if (!e->splitk_ws) { e->splitk_ws_bytes = 0; return false; }
    }
    const int Sp = round_up(S, 64), M = B * Sp, Mpad = round_up(M, 256);
    const size_t es = esize(e->dtype);
    const bool bert = c.backbone == GLC_BACKBONE_BERT, t5 = c.backbone == GLC_BACKBONE_T5;
    const bool dec = c.backbone == GLC_BACKBONE_DECODER || c.backbone == GLC_BACKBONE_MODERNBERT || bert || t5;    // (same workspace)
    const int nh_ws = t5 ? e->t5_heads : c.heads, nkv_ws = t5 ? e->t5_heads : c.kv_heads;      // (T5: the head count the kernels run)
    if (Mpad > e->capM) {
        const size_t rows_h = (size_t)Mpad * c.hidden * es;
        if (!regrow(e, e->X, rows_h) || !regrow(e, e->H1, rows_h) || !regrow(e, e->FF, (size_t)Mpad * c.inter * es) ||
            !regrow(e, e->kbias, (size_t)Mpad * sizeof(float))) return false;
        // (mean, rstd) or (0, rstd) per row of the two residual-stream buffers + the producers' partials (small; DeBERTa keeps them whether or not
        // the fold is switched on: glc_debug_set_ln_fused; the decoder's RMSNorm fold exists in the fp32 mode only)
        if (bert && !regrow(e, e->pos_ids, (size_t)Mpad * sizeof(int))) return false;
        if ((!dec || e->dtype == GLC_F32) && !bert && !t5) {      // (BERT, T5: no norm fold)
            if (!regrow(e, e->statsA, (size_t)Mpad * sizeof(float2)) || !regrow(e, e->statsB, (size_t)Mpad * sizeof(float2)) ||
                !regrow(e, e->ln_part, (size_t)Mpad * ((c.hidden + 63) / 64) * sizeof(float2))) return false;
        }
        if (dec) {
            const size_t nqd = (size_t)nh_ws * c.head_dim, nkvd = (size_t)nkv_ws * c.head_dim;
            if (!regrow(e, e->X2, rows_h) || !regrow(e, e->QKV, (size_t)Mpad * (nqd + 2 * nkvd) * es) || !regrow(e, e->CTX, (size_t)Mpad * nqd * es)) return false;
            if (e->dtype != GLC_F32 || e->dec_split) {          // fragment-major operands of the MFMA attention kernel (fp32 mode: split-f16 units, same bytes)
                if (!regrow(e, e->Qh, (size_t)Mpad * nqd * es) || !regrow(e, e->Kh, (size_t)Mpad * nkvd * es) || !regrow(e, e->Vt, (size_t)Mpad * nkvd * es)) return false;
            }
            // [gate | up] rows: read only by the launches without the SwiGLU epilogue (unfused builds, the fp32 mode's small forwards) — allocated
            // by the forward that takes such a launch (gated_ffn), not for every capacity step (2.3 GB at c5 that the group-split pipeline never touches)
            dfree(e, e->GU); e->GU = nullptr; e->capGU = 0;
        } else {
            for (void** b : {&e->Qh, &e->Kh, &e->Vt, &e->CTX, &e->T1}) if (!regrow(e, *b, rows_h)) return false;
        }
        e->capM = Mpad;
        e->hidden_cap = 0;   // dump buffer is re-made lazily
    }
    if (B > e->capB || C > e->capC) {
        const int nb = B > e->capB ? B : e->capB, nc = C > e->capC ? C : e->capC;
        const size_t nbc = (size_t)nb * (nc > 0 ? nc : 1);
        if (!regrow(e, e->klen, (size_t)nb * sizeof(int)) || !regrow(e, e->kfirst, (size_t)nb * sizeof(int)) || !regrow(e, e->cls_cnt, (size_t)nb * sizeof(int)) ||
            !regrow(e, e->cls_pos, nbc * sizeof(int)) || !regrow(e, e->d_logits, nbc * sizeof(float))) return false;
        e->capB = nb; e->capC = nc;
    }
    if (B * S > e->capIds) {
        if (!regrow(e, e->d_ids, (size_t)B * S * sizeof(int64_t)) || !regrow(e, e->d_mask, (size_t)B * S * sizeof(int64_t))) return false;
        e->capIds = B * S;
    }
    const bool seqcls = c.head_kind == GLC_HEAD_SEQCLS;      // (its C is the label count: no class rows, neither in the head nor in the pruned last layer)
    const int hr = round_up(B, 128) + (seqcls ? 0 : round_up(B * (C > 0 ? C : 1), 128));      // text rows then class rows, each group 128-aligned
    if (hr > e->capHeadRows) {
        for (float** b : {&e->Gt, &e->G1t, &e->G2t}) if (!regrow(e, *b, (size_t)hr * c.hidden * sizeof(float))) return false;
        // weighted-dot: [hr, 2H] + [rc, 3H] + [rc, 4H]; mlp: [rc, 2H] + [rc, 256] + [rc, 128] (rc <= hr)
        if (c.scorer != GLC_SCORER_DOT && !regrow(e, e->scorer_ws, (size_t)hr * (9 * (size_t)c.hidden + 2 * GLC_SCORER_MLP_HIDDEN) * sizeof(float))) return false;
        e->capHeadRows = hr;
    }
    // compact rows of the pruned last layer (every backbone): R = B (1 + C) rows up to the 256-row grid of the small-M GEMMs; the decoder's
    // context rows are heads * head_dim wide, which need not be the hidden size
    const int rsel = round_up(B * (1 + (C > 0 && !seqcls ? C : 0)), 256);
    if (rsel > e->capSel && !bert) {       // (BERT: no pruned last layer)
        const size_t wide = dec ? std::max((size_t)c.hidden, (size_t)nh_ws * c.head_dim) : (size_t)c.hidden;
        for (void** b : {&e->Xs, &e->CTXs, &e->T1s, &e->H1s}) if (!regrow(e, *b, (size_t)rsel * wide * es)) return false;
        if (!dec && !regrow(e, e->Qs, (size_t)rsel * c.hidden * es)) return false;
        if (dec && !regrow(e, e->GUs, (size_t)rsel * 2 * c.inter * es)) return false;
        if (!regrow(e, e->FFs, (size_t)rsel * c.inter * es) || !regrow(e, e->sel_b, (size_t)rsel * sizeof(int)) || !regrow(e, e->sel_q, (size_t)rsel * sizeof(int))) return false;
        e->capSel = rsel;
    }
    const size_t nf = (size_t)Mpad >> 5;      // one byte per 32-row tile of the padded row grid (the QKV GEMM reads 8 per 256-row tile)
    if (nf > e->capFlag) {
        if (!regrow(e, e->tile_flag, nf)) return false;
        e->capFlag = nf;
    }
    if (t5 && !build_rpb_table(e, Sp)) return false;
    if (dec) return build_rope_tables(e, Sp);
    return build_position_tables(e, Sp);
}

// the scorer's tensors (after the 8 projector tensors): matrices that a GEMM reads are pre-split like the projectors', the last Linear
// (out features 1) stays a plain vector
bool upload_scorer(glc_engine* e, const float* const* t) {
    const int H = e->cfg.hidden, Mh = GLC_SCORER_MLP_HIDDEN;
    size_t n[8] = {0};
    bool mat[8] = {false};
    int cnt = 0;
    if (e->cfg.scorer == GLC_SCORER_WEIGHTED_DOT) {
        const size_t v[8] = {2 * (size_t)H * H, 2 * (size_t)H, 2 * (size_t)H * H, 2 * (size_t)H, 12 * (size_t)H * H, 4 * (size_t)H, 4 * (size_t)H, 1};
        for (int i = 0; i < 8; ++i) n[i] = v[i];
        mat[0] = mat[2] = mat[4] = true; cnt = 8;
    } else if (e->cfg.scorer == GLC_SCORER_MLP) {
        const size_t v[6] = {(size_t)Mh * 2 * H, (size_t)Mh, (size_t)Mh / 2 * Mh, (size_t)Mh / 2, (size_t)Mh / 2, 1};
        for (int i = 0; i < 6; ++i) n[i] = v[i];
        mat[0] = mat[2] = true; cnt = 6;
    }
    for (int i = 0; i < cnt; ++i) {
        e->scw[i] = upload_f32(e, t[i], n[i]);
        if (!e->scw[i]) return false;
        if (mat[i] && e->w_presplit) { const char* pm = glc_launch_presplit(e->stream, e->scw[i], n[i]); if (pm) { glc_set_err(pm); return false; } }
    }
    return true;
}

// GEMM launches of the forward carry the engine's split-K workspace (used only when a shape has too few tiles, gemm.hip)
static bool presplit_weight(const glc_engine* e, int dt, const void* W) {
    if (!e->w_presplit || dt != GLC_F32) return false;
    return true;                                                                 // head projectors and every layer weight of the fp32 mode
}
const char* launch_gemm_auto(glc_engine* e, int dt, int epi, GemmArgs a) {
    a.ws = e->splitk_ws; a.ws_bytes = e->splitk_ws_bytes; a.w_presplit = presplit_weight(e, dt, a.W);
    return glc_launch_gemm_auto(e->stream, dt, epi, a);
}
const char* launch_gemm128(glc_engine* e, int dt, int epi, GemmArgs a) {
    a.ws = e->splitk_ws; a.ws_bytes = e->splitk_ws_bytes; a.w_presplit = presplit_weight(e, dt, a.W);
    return glc_launch_gemm(e->stream, dt, epi, a);
}

// MX pipeline: the GX copies of the projection weights (hi f16 | fp8 parts, glc_common.h; each tensor with the fp8 exponent its largest
// magnitude allows), made on the device from the split-f16 (group-split) copies by the FIRST forward that takes the pipeline — an engine
// whose forwards never reach the 256-tile pipeline (the reference's own batches of 8 short texts) never pays their memory.
// (the body; `made` collects every pointer slot it fills so that build_mx_weights can undo a partial build)
static bool build_mx_weights_impl(glc_engine* e, std::vector<void**>& made) {
    unsigned* d_bits = (unsigned*)e->splitk_ws;          // (scratch: the split-K workspace is idle between launches)
    if (!d_bits) { glc_set_err("MX weights: no scratch"); return false; }
    auto copy = [&](const void* gs, size_t n, void*& dst, int& ws) -> bool {
        if (!gs) { glc_set_err("MX weights: a split-f16 source copy is missing"); return false; }
        unsigned bits = 0;
        HIPCHK(hipMemsetAsync(d_bits, 0, sizeof(unsigned), e->stream), false);
        KCHK(glc_launch_gs_absmax(e->stream, gs, n, d_bits), false);
        HIPCHK(hipMemcpyAsync(&bits, d_bits, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream), false);
        HIPCHK(hipStreamSynchronize(e->stream), false);
        float mxv; memcpy(&mxv, &bits, sizeof(float));
        ws = glc_gx_weight_exponent(mxv);
        dst = dmalloc(e, n * sizeof(float), false);
        if (!dst) return false;
        made.push_back(&dst);
        KCHK(glc_launch_gs_to_gx(e->stream, gs, dst, n, ws), false);
        e->mx_bytes += n * sizeof(float);
        return true;
    };
    const glc_model_config& c = e->cfg;
    const size_t H = c.hidden, I = c.inter;
    if (c.backbone == GLC_BACKBONE_DECODER) {
        const size_t NQ = (size_t)c.heads * c.head_dim, NQKV = NQ + 2 * (size_t)c.kv_heads * c.head_dim;
        // RoPE + MX tiles as the epilogue of the QKV projection (gemm256x EPI_QKVR; head_dim 128, even head counts): the rows of every Q / K head
        // of the GX copy (and a copy of the bias) go into the order glc_rope_perm128 names — 32-row blocks 1 and 2 of the head trade places
        const bool rope_epi = e->dec_rope_epi && c.head_dim == 128 && c.heads % 2 == 0 && c.kv_heads % 2 == 0;
        void* tmp = nullptr;
        struct TmpGuard { glc_engine* e; void*& p; ~TmpGuard() { if (p) { (void)hipStreamSynchronize(e->stream); dfree(e, p); p = nullptr; } } } tmp_guard{e, tmp};      // (every exit path)
        const size_t blk = (size_t)32 * H * sizeof(float);        // 32 GX rows
        if (rope_epi) { tmp = dmalloc(e, blk, false); if (!tmp) return false; }
        for (auto& w : e->dlayers) {
            if (!copy(w.Wqkvf, NQKV * H, w.Wqkvf_x, w.ws_qkvf) || !copy(w.Wo, H * NQ, w.Wo_x, w.ws_o) ||
                !copy(w.Wguf, 2 * I * H, w.Wguf_x, w.ws_guf) || !copy(w.Wd, H * I, w.Wd_x, w.ws_d)) return false;
            if (!rope_epi) continue;
            if (w.bqkv) {                                     // (no biases — Llama, Qwen3 — no permuted copy: the permuted weight alone says so)
                w.bqkv_p = (float*)dmalloc(e, NQKV * sizeof(float), false);
                if (!w.bqkv_p) return false;
                made.push_back(reinterpret_cast<void**>(&w.bqkv_p));
                HIPCHK(hipMemcpyAsync(w.bqkv_p, w.bqkv, NQKV * sizeof(float), hipMemcpyDeviceToDevice, e->stream), false);
            }
            w.qkv_perm = true;
            for (int hd = 0; hd < c.heads + c.kv_heads; ++hd) {
                char* r1 = (char*)w.Wqkvf_x + ((size_t)hd * 128 + 32) * H * sizeof(float);
                char* r2 = r1 + blk;
                HIPCHK(hipMemcpyAsync(tmp, r1, blk, hipMemcpyDeviceToDevice, e->stream), false);
                HIPCHK(hipMemcpyAsync(r1, r2, blk, hipMemcpyDeviceToDevice, e->stream), false);
                HIPCHK(hipMemcpyAsync(r2, tmp, blk, hipMemcpyDeviceToDevice, e->stream), false);
                if (!w.bqkv_p) continue;
                HIPCHK(hipMemcpyAsync(w.bqkv_p + hd * 128 + 32, w.bqkv + hd * 128 + 64, 32 * sizeof(float), hipMemcpyDeviceToDevice, e->stream), false);
                HIPCHK(hipMemcpyAsync(w.bqkv_p + hd * 128 + 64, w.bqkv + hd * 128 + 32, 32 * sizeof(float), hipMemcpyDeviceToDevice, e->stream), false);
            }
        }
    } else if (c.backbone == GLC_BACKBONE_MODERNBERT) {
        // (no norm fold on this backbone: the unfolded Wqkv / Wo / Wi / mlp.Wo; Wi keeps its interleaved 16 input / 16 gate rows)
        for (auto& w : e->dlayers)
            if (!copy(w.Wqkv, 3 * H * H, w.Wqkv_x, w.ws_qkv) || !copy(w.Wo, H * H, w.Wo_x, w.ws_o) ||
                !copy(w.Wgu, 2 * I * H, w.Wgu_x, w.ws_gu) || !copy(w.Wd, H * I, w.Wd_x, w.ws_d)) return false;
    } else {
        for (size_t l = 0; l < e->layers.size(); ++l) {
            LayerW& w = e->layers[l];
            if (!copy(w.Wqkv, 3 * H * H, w.Wqkv_x, w.ws_qkv) || !copy(w.Wo, H * H, w.Wo_x, w.ws_o) || !copy(w.W2, H * I, w.W2_x, w.ws_2) ||
                !copy(w.W1f, I * H, w.W1f_x, w.ws_1f)) return false;
            if (l > 0 && !copy(w.Wqkvf, 3 * H * H, w.Wqkvf_x, w.ws_qkvf)) return false;
        }
    }
    HIPCHK(hipStreamSynchronize(e->stream), false);
    return true;
}

// The GX copies of the projection weights (+0.4 / 1.4 / 5.2 GB for base / large / the Qwen2-1.5B shape), built by the first forward that takes the
// MX pipeline.  A failure (out of memory, most likely) must not fail that forward, leak per call or leave a layer half converted:
// whatever this call allocated is freed, the pointers are cleared, and the engine stays on the split-f16 kernels (as GLICLASS_MX=0) from then on.
bool build_mx_weights(glc_engine* e) {
    if (e->mx_ready) return true;
    if (!e->mx_built) return false;
    std::vector<void**> made;
    if (build_mx_weights_impl(e, made)) { e->mx_ready = true; return true; }
    (void)hipStreamSynchronize(e->stream);
    (void)hipGetLastError();
    for (void** slot : made) { dfree(e, *slot); *slot = nullptr; }
    for (auto& w : e->dlayers) w.qkv_perm = false;
    e->mx_bytes = 0;
    e->mx_built = false;
    e->mx = false;
    fprintf(stderr, "gliclass: the MX weight copies could not be built (%s); this engine keeps the split-f16 arithmetic (as GLICLASS_MX=0)\n", glc_last_error());
    return false;
}

// The head after the row gather: the two FeaturesProjectors (Linear -> GELU -> Linear; text rows [0, rt) and class rows [rt, rt + rc)
// share one fp32 buffer, one two-group GEMM per stage), then the scorer (include/gliclass_hip.h).
bool run_head_tail(glc_engine* e, int B, int C, float* d_logits) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden;
    hipStream_t st = e->stream;
    const int rt = round_up(B, 128), rc = round_up(B * C, 128);
    GemmArgs h;
    h.N = H; h.K = H; h.Mpad = rt + rc; h.m_split = rt;
    h.A = e->Gt; h.W = e->headw[0]; h.bias = e->headw[1]; h.W2 = e->headw[4]; h.bias2 = e->headw[5]; h.C = e->G1t;
    KCHK(launch_gemm128(e, GLC_F32, EPI_GELU, h), false);
    h.A = e->G1t; h.W = e->headw[2]; h.bias = e->headw[3]; h.W2 = e->headw[6]; h.bias2 = e->headw[7]; h.C = e->G2t;
    KCHK(launch_gemm128(e, GLC_F32, EPI_BIAS, h), false);
    const float* Tt = e->G2t;
    const float* Cc = e->G2t + (size_t)rt * H;
    // normalize_features (upstream: projected text and class features are L2-normalised before ANY scorer and the logits multiplied by
    // logit_scale): the dot scorer does both inside its kernel; the other scorers get a row pass over G2 and the scale in their last step
    const float lscale = c.normalize_features ? c.logit_scale : 1.0f;
    if (c.scorer != GLC_SCORER_DOT && c.normalize_features) KCHK(glc_launch_l2norm_rows(st, e->G2t, rt + rc, H), false);
    if (c.scorer == GLC_SCORER_DOT) {
        KCHK(glc_launch_head_score(st, Tt, Cc, d_logits, B, C, H, c.normalize_features, c.logit_scale), false);
    } else if (c.scorer == GLC_SCORER_WEIGHTED_DOT) {
        float* S1 = e->scorer_ws;                                // [rt + rc, 2H]: proj_text on the text rows, proj_label on the class rows
        float* cat = S1 + (size_t)(rt + rc) * 2 * H;             // [rc, 3H]
        float* hid = cat + (size_t)rc * 3 * H;                   // [rc, 4H]
        GemmArgs g;
        g.N = 2 * H; g.K = H; g.Mpad = rt + rc; g.m_split = rt;
        g.A = e->G2t; g.W = e->scw[0]; g.bias = e->scw[1]; g.W2 = e->scw[2]; g.bias2 = e->scw[3]; g.C = S1;
        KCHK(launch_gemm128(e, GLC_F32, EPI_BIAS, g), false);
        KCHK(glc_launch_scorer_wd_cat(st, S1, S1 + (size_t)rt * 2 * H, cat, B, C, H), false);
        GemmArgs o;
        o.N = 4 * H; o.K = 3 * H; o.Mpad = rc; o.A = cat; o.W = e->scw[4]; o.bias = e->scw[5]; o.C = hid;
        KCHK(launch_gemm128(e, GLC_F32, EPI_BIAS, o), false);
        KCHK(glc_launch_relu_dot(st, hid, e->scw[6], e->scw[7], d_logits, B * C, 4 * H, lscale), false);
    } else {
        const int Mh = GLC_SCORER_MLP_HIDDEN;
        float* pair = e->scorer_ws;                              // [rc, 2H] = [text | class]
        float* h1 = pair + (size_t)rc * 2 * H;                   // [rc, 256]
        float* h2 = h1 + (size_t)rc * Mh;                        // [rc, 128]
        KCHK(glc_launch_scorer_pair(st, Tt, Cc, pair, B, C, H), false);
        GemmArgs g;
        g.N = Mh; g.K = 2 * H; g.Mpad = rc; g.A = pair; g.W = e->scw[0]; g.bias = e->scw[1]; g.C = h1;
        KCHK(launch_gemm128(e, GLC_F32, EPI_BIAS, g), false);
        KCHK(glc_launch_relu(st, h1, (size_t)rc * Mh), false);
        GemmArgs g2;
        g2.N = Mh / 2; g2.K = Mh; g2.Mpad = rc; g2.A = h1; g2.W = e->scw[2]; g2.bias = e->scw[3]; g2.C = h2;
        KCHK(launch_gemm128(e, GLC_F32, EPI_BIAS, g2), false);
        KCHK(glc_launch_relu_dot(st, h2, e->scw[4], e->scw[5], d_logits, B * C, Mh / 2, lscale), false);
    }
    return true;
}

inline int class_cap(const glc_engine* e) { return e->capC > 0 ? e->capC : 1; }
// class-token rows per text that the head reads (the pruned last layers keep them): none for the sequence-classification head, whose C counts labels
inline int class_rows(const glc_engine* e, int C) { return e->cfg.head_kind == GLC_HEAD_SEQCLS || C < 0 ? 0 : C; }

// The sequence-classification head on the B pooled rows in Gt (cls_head.hip has the arithmetic and its sources): the dense stage on the GEMM path
// of the GLiClass projectors (fp32 rows, split-f16 weights), then activation, norm, classifier and bias in one launch -> logits [B, K]
bool run_cls_head(glc_engine* e, int B, float* d_logits) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden;
    const float* x = e->Gt;
    if (c.cls_dense) {
        GemmArgs h;
        h.N = H; h.K = H; h.Mpad = round_up(B, 128);
        h.A = e->Gt; h.W = e->clsw[0]; h.bias = e->clsw[1]; h.C = e->G1t;
        KCHK(launch_gemm128(e, GLC_F32, EPI_BIAS, h), false);
        x = e->G1t;
    }
    KCHK(glc_launch_cls_head(e->stream, x, c.cls_norm ? e->clsw[2] : nullptr, c.cls_norm ? e->clsw[3] : nullptr, e->clsw[4], e->clsw[5], d_logits,
                             B, H, c.cls_labels, c.cls_act, c.ln_eps), false);
    return true;
}

// The start of every forward: profiler reset, the hidden-state dump buffer (keep_hidden: L + 1 slots of M rows), scan_rows.
bool forward_prologue(glc_engine* e, const int64_t* ids, const int64_t* mask, int B, int S) {
    const glc_model_config& c = e->cfg;
    if (e->profile) e->ev_used = 0;
    if (e->keep_hidden) {
        const size_t need = (size_t)(c.layers + 1) * B * round_up(S, 64) * c.hidden * esize(e->dtype);
        if (need > e->hidden_cap) { dfree(e, e->hidden_dump); e->hidden_dump = dmalloc(e, need); if (!e->hidden_dump) return false; e->hidden_cap = need; }
    }
    Prof p(e, PC_SCAN);
    KCHK(glc_launch_scan_rows(e->stream, ids, mask, B, S, c.class_token_index, c.embed_class_token, e->klen, e->kfirst, e->cls_pos, e->cls_cnt, class_cap(e)), false);
    return true;
}

// keep_hidden: the M rows at src into slot `slot` of the dump buffer (0: embedding output, l + 1: output of layer l, L: the final rows)
bool dump_hidden(glc_engine* e, int slot, const void* src, int M) {
    if (!e->keep_hidden) return true;
    const size_t n = (size_t)M * e->cfg.hidden * esize(e->dtype);
    HIPCHK(hipMemcpyAsync((char*)e->hidden_dump + slot * n, src, n, hipMemcpyDeviceToDevice, e->stream), false);
    return true;
}

// The end of every forward: the head reads `rows` — the final rows of the backbone (gather + pooling), or the compact rows of
// DeBERTa's pruned last layer (one [CLS] row and C class-token rows per text) — then the projectors and the scorer.
bool forward_epilogue(glc_engine* e, const void* rows, bool compact, int B, int S, int C, float* d_logits) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, Sp = round_up(S, 64), dt = e->dtype;
    hipStream_t st = e->stream;
    if (c.head_kind == GLC_HEAD_SEQCLS) {      // pooled rows only (compact rows: row b is text b's), then the classifier; C = cls_labels (checked by the entries)
        Prof p(e, PC_HEAD);
        if (compact) KCHK(glc_launch_head_gather_sel(st, dt, rows, e->cls_pos, class_cap(e), e->Gt, e->Gt, B, H, 0), false);
        else if (c.pooling == GLC_POOL_AVG) KCHK(glc_launch_pool_avg(st, dt, rows, e->kbias, e->Gt, B, Sp, H), false);
        else KCHK(glc_launch_head_gather(st, dt, rows, e->cls_pos, class_cap(e), e->Gt, e->Gt, B, Sp, H, 0, nullptr), false);
        if (!run_cls_head(e, B, d_logits)) return false;
    } else if (C > 0) {
        Prof p(e, PC_HEAD);
        float* Gc = e->Gt + (size_t)round_up(B, 128) * H;
        if (compact) KCHK(glc_launch_head_gather_sel(st, dt, rows, e->cls_pos, class_cap(e), e->Gt, Gc, B, H, C), false);
        else {
            KCHK(glc_launch_head_gather(st, dt, rows, e->cls_pos, class_cap(e), e->Gt, Gc, B, Sp, H, C, c.pooling == GLC_POOL_LAST ? e->klen : nullptr), false);
            if (c.pooling == GLC_POOL_AVG) KCHK(glc_launch_pool_avg(st, dt, rows, e->kbias, e->Gt, B, Sp, H), false);
        }
        if (!run_head_tail(e, B, C, d_logits)) return false;
    }
    HIPCHK(hipGetLastError(), false);
    e->lastB = B; e->lastS = S; e->lastSp = Sp;
    return true;
}

// The group-split projections of a forward: the 256-tile split-f16 kernel (gemm256s.hip), or on the MX pipeline the cross-term kernel on GX rows
// (small: glc_engine::mx_small — with it on, a launch of an MX forward that has too few 256-tiles for the device runs the 128 tile, gemm128x.hip;
//  n128 counts those launches)
struct GemmGs {
    hipStream_t st; bool mx; int M; int small = 0; int* n128 = nullptr;
    const char* operator()(int epi, const GemmArgs& a) const {
        if (!mx) return glc_launch_gemm256s_gs(st, epi, a);
        GemmArgs gx = a; gx.gx_rows = M;          // fp8 range guard: the M rows of this forward, not the slack rows up to Mpad
        if (small > 0 && glc_gemm_small_m(gx) && glc_gemm128x_supported(gx, epi)) {
            if (n128) ++*n128;
            return glc_launch_gemm128x(st, epi, gx);
        }
        return glc_launch_gemm256x(st, epi, gx);
    }
};

// The gated FFN's first projection and its gate: FF = act(first) * second (decoder: silu(gate) * up, ModernBERT: gelu(input) * gate).
// f1 = the [first | second] projection without its output (A, W, Mpad, N = 2I, K, the RMSNorm fold's operands); with the weight rows
// interleaved (fused_swiglu) the gate runs in the GEMM epilogue, else as a pass of its own over the GU rows.
struct Glu {
    int epi;                                                                          // EPI_SWIGLU / EPI_GEGLU
    const char* (*rows)(hipStream_t, int, const void*, void*, size_t, int, int);      // the gate over GU rows of T (last argument: interleaved columns)
    const char* (*rows_gs)(hipStream_t, const float*, void*, size_t, int);            // ... over plain fp32 GU rows, group-split output
};
const Glu kSwiGlu{EPI_SWIGLU, glc_launch_swiglu, glc_launch_swiglu_gs}, kGeGlu{EPI_GEGLU, glc_launch_geglu, glc_launch_geglu_gs};
// T5's gated tanh-GELU: a row pass only (the backbone runs with fused_swiglu = false; there is no tanh-GELU GEMM epilogue, so epi is never read)
const Glu kGeGluTanh{EPI_GEGLU, glc_launch_geglu_tanh, glc_launch_geglu_tanh_gs};

bool gated_ffn(glc_engine* e, const Glu& glu, GemmArgs f1, bool gs, const GemmGs& gemm_gs, int M) {
    hipStream_t st = e->stream;
    const int dt = e->dtype, I = e->cfg.inter;
    const bool fused = e->fused_swiglu;
    // [first | second] rows: written only by the launches without the gate epilogue, allocated by the first forward that takes one
    if (!(fused && (gs || dt != GLC_F32)) && e->capGU < f1.Mpad) {
        dfree(e, e->GU); e->GU = dmalloc(e, (size_t)f1.Mpad * 2 * I * esize(dt));
        if (!e->GU) return false;
        e->capGU = f1.Mpad;
    }
    f1.C = e->GU;
    Prof p(e, PC_FFN1);
    if (fused && gs) { f1.C = e->FF; KCHK(gemm_gs(glu.epi, f1), false); }
    else if (fused && dt == GLC_F32) {      // small forward of the fp32 mode: plain rows, interleaved columns
        KCHK(launch_gemm_auto(e, dt, EPI_BIAS, f1), false); KCHK(glu.rows(st, dt, e->GU, e->FF, (size_t)M, I, 1), false); }
    else if (fused) { f1.C = e->FF; KCHK(glc_launch_gemm256s(st, dt, glu.epi, f1), false); }
    else if (gs) { f1.gs_c_plain = 1; KCHK(gemm_gs(EPI_BIAS, f1), false); KCHK(glu.rows_gs(st, (const float*)e->GU, e->FF, (size_t)M, I), false); }
    else { KCHK(launch_gemm_auto(e, dt, EPI_BIAS, f1), false); KCHK(glu.rows(st, dt, e->GU, e->FF, (size_t)M, I, 0), false); }
    return true;
}

// Exact pruning of the last layer on the pre-norm backbones (decoder, ModernBERT) — the scheme of run_forward_deberta's band_sel branch.  The head
// reads R = B (1 + C) rows: the pooled row of every sequence (position 0, or klen - 1 with 'last' pooling) and its class-token rows.  K and V
// of the last layer are needed at every position, so its norm, QKV projection and RoPE / layout pass run on all rows as in any layer; the
// attention runs on the 32-query tiles that hold a selected row (tile_flag, written by the row gather), and everything behind it — context
// gather, o-projection with the compact residual, norm, gated FFN, the final norm — on the R compact rows, plain rows of T on the
// small-M kernels.  Average pooling reads every row and keep_hidden dumps every row: never pruned.
struct PrunedTail {
    bool on = false;
    int R = 0, Rpad = 0, Cc = 0;
    const int* klen = nullptr;        // 'last' pooling: the pooled row is klen - 1
};
PrunedTail pruned_tail(const glc_engine* e, int B, int C) {
    PrunedTail t;
    const glc_model_config& c = e->cfg;
    t.on = e->prune_last && !e->keep_hidden && (c.pooling == GLC_POOL_FIRST || c.pooling == GLC_POOL_LAST) && c.layers > 0;
    t.Cc = class_rows(e, C);
    t.R = B * (1 + t.Cc); t.Rpad = round_up(t.R, 256);
    t.klen = c.pooling == GLC_POOL_LAST ? e->klen : nullptr;
    return t;
}
// The compact rows behind the attention: Xs = the residual rows (gathered ahead of the layer), CTXs = the context rows.  norm(src, dst, gain)
// is the backbone's norm over R rows; the head reads H1s, the final norm of the R rows (forward_epilogue, compact).
template <class Norm>
bool run_pruned_tail(glc_engine* e, const PrunedTail& t, const DecLayerW& w, const Glu& glu, int NQ, const Norm& norm) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter, dt = e->dtype;
    GemmArgs o;
    o.A = e->CTXs; o.W = w.Wo; o.bias = nullptr; o.C = e->T1s; o.resid = e->Xs; o.Mpad = t.Rpad; o.N = H; o.K = NQ;
    KCHK(launch_gemm_auto(e, dt, EPI_RESID, o), false);
    KCHK(norm(e->T1s, e->H1s, w.ln2), false);
    GemmArgs f1;      // the resident [first | second] weight (interleaved rows where the full layers gate in their epilogue), the gate as a row pass
    f1.A = e->H1s; f1.W = w.Wgu; f1.bias = nullptr; f1.C = e->GUs; f1.Mpad = t.Rpad; f1.N = 2 * I; f1.K = H;
    KCHK(launch_gemm_auto(e, dt, EPI_BIAS, f1), false);
    KCHK(glu.rows(e->stream, dt, e->GUs, e->FFs, (size_t)t.R, I, e->fused_swiglu ? 1 : 0), false);
    GemmArgs f2;
    f2.A = e->FFs; f2.W = w.Wd; f2.bias = nullptr; f2.C = e->Xs; f2.resid = e->T1s; f2.Mpad = t.Rpad; f2.N = H; f2.K = I;
    KCHK(launch_gemm_auto(e, dt, EPI_RESID, f2), false);
    KCHK(norm(e->Xs, e->H1s, e->final_norm), false);
    e->last_pruned = true;
    return true;
}

// Decoder-style backbone: one launch sequence per batch (Q2:384-398).  Pre-norm residual stream X (operand type T).
bool run_forward_decoder(glc_engine* e, const int64_t* ids, const int64_t* mask, int B, int S, int C, float* d_logits) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter, nq = c.heads, nkv = c.kv_heads, d = c.head_dim, L = c.layers;
    const int NQ = nq * d, NQKV = (nq + 2 * nkv) * d;
    const int Sp = round_up(S, 64), M = B * Sp, Mpad = round_up(M, 256);
    hipStream_t st = e->stream;
    const int dt = e->dtype;
    const size_t es = esize(dt);
    GxScope gx_scope(e);                     // fp8 range guard + activation exponent: the launchers of this thread hand them to every producer / reader of GX rows and MX tiles
    if (!forward_prologue(e, ids, mask, B, S)) return false;
    { Prof p(e, PC_EMBED);
      KCHK(glc_launch_embed_plain(st, dt, ids, mask, e->emb, e->X, e->kbias, B, S, Sp, H, c.vocab, c.pad_id), false); }
    if (!dump_hidden(e, 0, e->X, M)) return false;
    const float qscale = 1.4426950408889634f / sqrtf((float)d);         // Q2:186 scaling, times log2(e) for the exp2 softmax
    const bool mfma = (dt != GLC_F32 || e->dec_split) && e->attn_impl != 1;   // flash-style MFMA kernel (fp32 mode: on split-f16 units); impl 1 / native fp32: straightforward kernel
    // group-split pipeline of the fp32 mode (see run_forward_deberta): the GEMM A operands (RMSNorm outputs, context rows, SwiGLU output) are
    // written as [32 hi | 32 lo] groups by their producers and every projection runs on the 256-tile LDS-DMA kernel; the residual
    // stream X, the fused QKV rows (RoPE / layout pass) and the [gate | up] rows stay plain fp32
    bool gs = false;
    if (dt == GLC_F32 && e->gs_mode > 0 && e->w_presplit && e->dec_split && mfma && !e->keep_hidden && H % 256 == 0 && (2 * I) % 256 == 0 &&
        NQKV % 256 == 0 && NQ % 32 == 0 && I % 32 == 0) {
        GemmArgs t; t.Mpad = Mpad; t.N = H; t.K = H;
        gs = e->gs_mode == 2 || !glc_gemm_small_m(t);
    }
    e->last_gs = gs;
    void *X = e->X, *Xn = e->X2;
    // RMSNorm folded away (group-split pipeline, e->ln_fused; docs/LOG_r01-r05.md §3d): the residual stream is kept as RAW group-split rows plus
    // (0, rstd) per row — statsA for the buffer X points at, statsB for the other — the projections run on weights with the RMSNorm gain
    // folded in and scale their accumulators by rstd in the epilogue; the residual GEMMs emit the partials of the next statistics.
    const bool rnf = gs && e->ln_fused && e->fused_swiglu && L > 0 && e->dlayers[0].Wqkvf && e->dlayers[0].Wguf && e->statsA && e->statsB && e->ln_part;
    float2 *sX = e->statsA, *sXn = e->statsB;
    e->last_lnf = rnf;
    // MX pipeline (round 3, as the encoder's): GX rows + gemm256x for the four projections of every layer; attention stays on split units
    bool mx = rnf && e->mx && e->mx_built && e->prec_mask == 0;
    if (mx && !build_mx_weights(e)) mx = false;          // (no copies: this and every later forward stay on the split-f16 kernels)
    for (int l = 0; mx && l < L; ++l) mx = e->dlayers[l].Wqkvf_x && e->dlayers[l].Wo_x && e->dlayers[l].Wguf_x && e->dlayers[l].Wd_x;
    e->last_mx = mx;
    e->last_mx128 = 0;
    const bool mxa = mx && mfma && e->mx_attn;      // round 4: the attention of the MX pipeline on MX tiles too (decoder_mx.hip)
    e->last_mx_attn = mxa;
    e->last_rope_epi = false;
    const GemmGs gemm_gs{st, mx, M};
    const PrunedTail pt = pruned_tail(e, B, C);
    e->last_pruned = false;
    if (rnf) {      // the embedding rows enter the pipeline: plain fp32 (X2) -> raw group-split rows (X) + statistics
        HIPCHK(hipMemcpyAsync(e->X2, e->X, (size_t)M * H * es, hipMemcpyDeviceToDevice, st), false);
        KCHK(glc_launch_rows_to_gs_rms(st, (const float*)e->X2, e->X, sX, c.ln_eps, M, H, mx ? 1 : 0), false);
    }
    for (int l = 0; l < L; ++l) {
        const DecLayerW& w = e->dlayers[l];
        const bool last = pt.on && l == L - 1;        // pruned: norm, QKV and RoPE on every row (K, V), attention on the flagged tiles, the rest compact
        const unsigned char* flag = last && mfma ? e->tile_flag : nullptr;      // (the straightforward kernel runs every row)
        if (last) {       // the rows the head reads: the residual stream as plain rows of T (the folded pipeline's raw rows come back as fp32)
            Prof p(e, PC_LAST);
            HIPCHK(hipMemsetAsync(e->tile_flag, 0, (size_t)Mpad >> 5, st), false);
            KCHK(rnf ? glc_launch_gather_rows_gs(st, X, e->cls_pos, class_cap(e), (float*)e->Xs, e->sel_b, e->sel_q, e->tile_flag, B, Sp, H, pt.Cc, mx ? 1 : 0, pt.klen)
                     : glc_launch_gather_rows(st, dt, X, e->cls_pos, class_cap(e), e->Xs, e->sel_b, e->sel_q, e->tile_flag, B, Sp, H, pt.Cc, pt.klen), false);
        }
        if (!rnf) { Prof p(e, last ? PC_LAST : PC_LN); KCHK(gs ? glc_launch_rmsnorm_gs(st, (const float*)X, e->H1, w.ln1, c.ln_eps, M, H)
                                    : glc_launch_rmsnorm(st, dt, X, e->H1, w.ln1, c.ln_eps, M, H), false); }                        // Q2:280
        GemmArgs g;
        g.A = e->H1; g.W = w.Wqkv; g.bias = w.bqkv; g.C = e->QKV; g.Mpad = Mpad; g.N = NQKV; g.K = H; g.gs_c_plain = 1;
        if (rnf) { g.A = X; g.W = w.Wqkvf; g.a_stats = sX; }
        if (mx) { g.W = w.Wqkvf_x; g.mx_ws = w.ws_qkvf; }
        const bool perm = mx && w.qkv_perm;          // Wqkvf_x rows in the RoPE-epilogue order (bqkv_p with them, null for a bias-free model)
        if (perm) { g.bias = w.bqkv_p; g.perm_cols = (nq + nkv) * d; }
        // Q2:206-211 in one launch: projection, RoPE, scale, MX tiles (gemm256x.hip EPI_QKVR).  Not with qk_norm (Qwen3, Q3:237-238): the norm
        // needs a head's 128 columns together and the epilogue holds them in more than one wave's sub-tile, so the plain projection (its
        // epilogue puts the permuted columns back) and the layout pass below, which carries the norm, run instead: one more pass over
        // the QKV rows per layer on the MX pipeline, for Qwen3 only (not measured).
        const bool rope_epi = perm && mxa && !c.qk_norm;
        if (l == 0) e->last_rope_epi = rope_epi;
        if (rope_epi) { g.rope_cs = e->ropes[{Sp, c.rope_theta}]; g.qscale = qscale; g.nq = nq; g.nkv = nkv; g.Sp = Sp; g.Mvalid = M; g.Qh = e->Qh; g.Kh = e->Kh; g.Vt = e->Vt; }
        { Prof p(e, last ? PC_LAST : PC_QKV);
          if (rope_epi) KCHK(gemm_gs(EPI_QKVR, g), false);
          else {
          KCHK(gs ? gemm_gs(EPI_BIAS, g) : launch_gemm_auto(e, dt, EPI_BIAS, g), false);        // Q2:206-208
          // (w.qn / w.kn: Qwen3's per-head RMSNorm, Q3:237-238, inside whichever of the three passes runs; null otherwise)
          if (mxa) KCHK(glc_launch_qkv_layout_mx(st, e->QKV, e->ropes[{Sp, c.rope_theta}], e->Qh, e->Kh, e->Vt, B, Sp, nq, nkv, d, qscale, w.qn, w.kn, c.ln_eps), false);     // Q2:211 RoPE, MX tiles (decoder_mx.hip)
          else if (mfma) KCHK(glc_launch_qkv_layout(st, dt, e->QKV, e->ropes[{Sp, c.rope_theta}], e->Qh, e->Kh, e->Vt, B, Sp, nq, nkv, d, qscale, w.qn, w.kn, c.ln_eps), false);   // Q2:211 RoPE
          else KCHK(glc_launch_rope_qk(st, dt, e->QKV, e->ropes[{Sp, c.rope_theta}], M, Sp, nq, nkv, d, qscale, w.qn, w.kn, c.ln_eps), false); } }
        { Prof p(e, last ? PC_LAST : PC_ATTN);
          if (mxa) KCHK(glc_launch_attention_gqa_mx(st, e->Qh, e->Kh, e->Vt, e->kbias, e->klen, e->kfirst, e->CTX, B, Sp, nq, nkv, d, c.causal, flag), false);
          else if (mfma) KCHK(glc_launch_attention_gqa_mfma(st, dt, e->Qh, e->Kh, e->Vt, e->kbias, e->klen, e->kfirst, e->CTX, B, Sp, nq, nkv, d, c.causal, last ? 0 : (mx ? 2 : (gs ? 1 : 0)), 0, flag), false);
          else KCHK(glc_launch_attention_gqa(st, dt, 1, e->QKV, e->kbias, e->klen, e->CTX, B, Sp, nq, nkv, d, c.causal), false); }
        if (last) {
            { Prof p(e, PC_LAST);
            // context rows of the selection: plain rows of T, or on MX tiles GX rows (the kernel has no other output), which the group-split gather
            // turns into fp32 (it writes the same row lists once more)
            KCHK(mxa ? glc_launch_gather_rows_gs(st, e->CTX, e->cls_pos, class_cap(e), (float*)e->CTXs, e->sel_b, e->sel_q, nullptr, B, Sp, NQ, pt.Cc, 1, pt.klen)
                     : glc_launch_gather_sel(st, dt, e->CTX, e->sel_b, e->sel_q, e->CTXs, pt.R, Sp, NQ), false);
            auto norm = [&](const void* src, void* dst, const float* gain) { return glc_launch_rmsnorm(st, dt, src, dst, gain, c.ln_eps, pt.R, H); };
            if (!run_pruned_tail(e, pt, w, kSwiGlu, NQ, norm)) return false; }                                                   // Q2:233-398 on R rows
            return forward_epilogue(e, e->H1s, true, B, S, C, d_logits);
        }
        GemmArgs o;
        o.A = e->CTX; o.W = w.Wo; o.bias = nullptr; o.C = Xn; o.resid = X; o.Mpad = Mpad; o.N = H; o.K = NQ; o.gs_resid_plain = 1;
        if (rnf) { o.gs_resid_plain = 0; o.ln_part = e->ln_part; }        // raw group-split residual in, raw group-split sum + partials out
        if (mx) { o.W = w.Wo_x; o.mx_ws = w.ws_o; }
        { Prof p(e, PC_ATTN_OUT); KCHK(gs ? gemm_gs(EPI_RESID, o) : launch_gemm_auto(e, dt, EPI_RESID, o), false); }   // Q2:233, :291
        std::swap(X, Xn); std::swap(sX, sXn);
        { Prof p(e, PC_LN); KCHK(rnf ? glc_launch_ln_stats(st, e->ln_part, H / 64, sX, M, H, c.ln_eps, 1)
                                 : gs ? glc_launch_rmsnorm_gs(st, (const float*)X, e->H1, w.ln2, c.ln_eps, M, H)
                                      : glc_launch_rmsnorm(st, dt, X, e->H1, w.ln2, c.ln_eps, M, H), false); }                        // Q2:295
        GemmArgs f1;
        f1.A = e->H1; f1.W = w.Wgu; f1.bias = nullptr; f1.Mpad = Mpad; f1.N = 2 * I; f1.K = H;
        if (rnf) { f1.A = X; f1.W = w.Wguf; f1.a_stats = sX; }
        if (mx) { f1.W = w.Wguf_x; f1.mx_ws = w.ws_guf; }
        if (!gated_ffn(e, kSwiGlu, f1, gs, gemm_gs, M)) return false;                                                          // Q2:47 silu(gate) * up
        GemmArgs f2;
        f2.A = e->FF; f2.W = w.Wd; f2.bias = nullptr; f2.C = Xn; f2.resid = X; f2.Mpad = Mpad; f2.N = H; f2.K = I; f2.gs_resid_plain = 1;
        if (rnf) { f2.gs_resid_plain = 0; if (l + 1 < L) f2.ln_part = e->ln_part; }      // (the last layer hands plain fp32 rows to the final norm)
        if (mx) { f2.W = w.Wd_x; f2.mx_ws = w.ws_d; }
        { Prof p(e, PC_FFN2); KCHK(gs ? gemm_gs(EPI_RESID, f2) : launch_gemm_auto(e, dt, EPI_RESID, f2), false); }
        std::swap(X, Xn); std::swap(sX, sXn);
        if (rnf && l + 1 < L) { Prof p(e, PC_LN); KCHK(glc_launch_ln_stats(st, e->ln_part, H / 64, sX, M, H, c.ln_eps, 1), false); }
        if (l + 1 < L && !dump_hidden(e, l + 1, X, M)) return false;
    }
    { Prof p(e, PC_LN); KCHK(glc_launch_rmsnorm(st, dt, X, e->H1, e->final_norm, c.ln_eps, M, H), false); }                    // Q2:398
    if (!dump_hidden(e, L, e->H1, M)) return false;
    return forward_epilogue(e, e->H1, false, B, S, C, d_logits);
}

// ModernBERT backbone (transformers models/modernbert/modeling_modernbert.py, cited as MB:<line>): one launch sequence per batch.
// Pre-norm residual stream X (operand type T; plain fp32 rows in the fp32 mode), bias-free LayerNorms (beta = e->zero_bias),
// bidirectional attention with RoPE, the local layers on the windowed attention kernels, GeGLU.  The fp32 mode's group-split pipeline
// runs with the norms as kernels of their own (no fold).  The MX pipeline is opt-in here (glc_engine_enable_mx / GLICLASS_MX_MODERNBERT=1):
// the same launch sequence with the norm, context and GeGLU rows as GX rows, the four projections on gemm256x (GeGLU in its epilogue) and
// the attention on MX tiles — the ring kernel on the global layers, the windowed per-wave kernel on the local ones (decoder_mx.hip).
bool run_forward_modernbert(glc_engine* e, const int64_t* ids, const int64_t* mask, int B, int S, int C, float* d_logits) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter, nh = c.heads, d = c.head_dim, L = c.layers;
    const int Sp = round_up(S, 64), M = B * Sp, Mpad = round_up(M, 256);
    hipStream_t st = e->stream;
    const int dt = e->dtype;
    GxScope gx_scope(e);                     // fp8 range guard + activation exponent (see run_forward_decoder)
    if (!forward_prologue(e, ids, mask, B, S)) return false;
    void *X = e->X, *Xn = e->X2;
    { Prof p(e, PC_EMBED);                                                                                                   // MB:52-71
      KCHK(glc_launch_embed_plain(st, dt, ids, mask, e->emb, Xn, e->kbias, B, S, Sp, H, c.vocab, c.pad_id), false);
      KCHK(glc_launch_layernorm(st, dt, Xn, X, e->eln_g, e->zero_bias, c.ln_eps, M, H), false); }
    if (!dump_hidden(e, 0, X, M)) return false;
    const float qscale = 1.4426950408889634f / sqrtf((float)d);         // head_dim^-1/2, times log2(e) for the exp2 softmax
    const bool mfma = (dt != GLC_F32 || e->dec_split) && e->attn_impl != 1;
    // group-split pipeline of the fp32 mode (as the decoder's, without the norm fold): LayerNorm / context / GeGLU rows are written as
    // [32 hi | 32 lo] groups, every projection runs on the 256-tile LDS-DMA kernel; X, QKV and the [input | gate] rows stay plain fp32
    bool gs = false;
    if (dt == GLC_F32 && e->gs_mode > 0 && e->w_presplit && e->dec_split && mfma && !e->keep_hidden && H % 256 == 0 && (2 * I) % 256 == 0 &&
        (3 * H) % 256 == 0 && I % 32 == 0) {
        GemmArgs t; t.Mpad = Mpad; t.N = H; t.K = H;
        gs = e->gs_mode == 2 || !glc_gemm_small_m(t);
    }
    e->last_gs = gs;
    e->last_lnf = false;
    // MX pipeline (opt-in: glc_engine_enable_mx): GX rows + gemm256x for the four projections of every layer, attention on MX tiles
    bool mx = gs && e->mx && e->mx_built && e->fused_swiglu && e->prec_mask == 0;
    if (mx && !build_mx_weights(e)) mx = false;          // (no copies: this and every later forward stay on the split-f16 kernels)
    for (int l = 0; mx && l < L; ++l) mx = e->dlayers[l].Wqkv_x && e->dlayers[l].Wo_x && e->dlayers[l].Wgu_x && e->dlayers[l].Wd_x;
    e->last_mx = mx;
    const bool mxa = mx && e->mx_attn;       // attention on MX tiles too (decoder_mx.hip); else split-f16 units with GX context rows
    e->last_mx_attn = mxa;
    e->last_rope_epi = false;
    const int gxr = mx ? 1 : 0;
    const GemmGs gemm_gs{st, mx, M};
    const PrunedTail pt = pruned_tail(e, B, C);
    e->last_pruned = false;
    auto norm = [&](const void* src, const float* gamma) -> const char* {      // H1 = LN(src) (group-split rows in the gs pipeline, GX rows on the MX pipeline)
        return gs ? glc_launch_layernorm_gs(st, (const float*)src, e->H1, gamma, e->zero_bias, c.ln_eps, M, H, gxr)
                  : glc_launch_layernorm(st, dt, src, e->H1, gamma, e->zero_bias, c.ln_eps, M, H);
    };
    for (int l = 0; l < L; ++l) {
        const DecLayerW& w = e->dlayers[l];
        const bool glob = c.local_window <= 0 || l % (c.global_every > 0 ? c.global_every : 1) == 0;
        const int win = glob ? 0 : c.local_window;
        float* cs = e->ropes[{Sp, glob ? c.rope_theta : c.rope_theta_local}];
        const bool last = pt.on && l == L - 1;        // pruned (see run_pruned_tail): the residual rows the head reads, then K / V on every row
        const unsigned char* flag = last && mfma ? e->tile_flag : nullptr;
        if (last) {
            Prof p(e, PC_LAST);
            HIPCHK(hipMemsetAsync(e->tile_flag, 0, (size_t)Mpad >> 5, st), false);
            KCHK(glc_launch_gather_rows(st, dt, X, e->cls_pos, class_cap(e), e->Xs, e->sel_b, e->sel_q, e->tile_flag, B, Sp, H, pt.Cc, pt.klen), false);
        }
        // MB:326-331: attn_norm is the identity on layer 0 (the QKV projection reads the embedding norm's rows; as group-split rows in the
        // gs pipeline, where the same norm runs once more into H1)
        if (l > 0) { Prof p(e, last ? PC_LAST : PC_LN); KCHK(norm(X, w.ln1), false); }
        else if (gs) { Prof p(e, last ? PC_LAST : PC_LN); KCHK(glc_launch_layernorm_gs(st, (const float*)Xn, e->H1, e->eln_g, e->zero_bias, c.ln_eps, M, H, gxr), false); }
        GemmArgs g;
        g.A = (l == 0 && !gs) ? X : e->H1; g.W = w.Wqkv; g.bias = nullptr; g.C = e->QKV; g.Mpad = Mpad; g.N = 3 * H; g.K = H; g.gs_c_plain = 1;
        if (mx) { g.W = w.Wqkv_x; g.mx_ws = w.ws_qkv; }
        { Prof p(e, last ? PC_LAST : PC_QKV);
          KCHK(gs ? gemm_gs(EPI_BIAS, g) : launch_gemm_auto(e, dt, EPI_BIAS, g), false);                                      // MB:274-279
          if (mxa) KCHK(glc_launch_qkv_layout_mx(st, e->QKV, cs, e->Qh, e->Kh, e->Vt, B, Sp, nh, nh, d, qscale), false);     // MB:281-282 RoPE, MX tiles
          else if (mfma) KCHK(glc_launch_qkv_layout(st, dt, e->QKV, cs, e->Qh, e->Kh, e->Vt, B, Sp, nh, nh, d, qscale), false);   // MB:281-282 RoPE
          else KCHK(glc_launch_rope_qk(st, dt, e->QKV, cs, M, Sp, nh, nh, d, qscale), false); }
        { Prof p(e, last ? PC_LAST : PC_ATTN);                                                                                 // MB:284-297
          if (mxa) KCHK(glc_launch_attention_gqa_mx(st, e->Qh, e->Kh, e->Vt, e->kbias, e->klen, e->kfirst, e->CTX, B, Sp, nh, nh, d, 0, flag, win), false);
          else if (mfma) KCHK(glc_launch_attention_gqa_mfma(st, dt, e->Qh, e->Kh, e->Vt, e->kbias, e->klen, e->kfirst, e->CTX, B, Sp, nh, nh, d, 0, last ? 0 : (mx ? 2 : (gs ? 1 : 0)), win, flag), false);
          else KCHK(glc_launch_attention_gqa(st, dt, 1, e->QKV, e->kbias, e->klen, e->CTX, B, Sp, nh, nh, d, 0, win), false); }
        if (last) {
            { Prof p(e, PC_LAST);
            // (on MX tiles the context rows are GX rows — the kernel has no other output: the group-split gather turns the selection into fp32)
            KCHK(mxa ? glc_launch_gather_rows_gs(st, e->CTX, e->cls_pos, class_cap(e), (float*)e->CTXs, e->sel_b, e->sel_q, nullptr, B, Sp, H, pt.Cc, 1, pt.klen)
                     : glc_launch_gather_sel(st, dt, e->CTX, e->sel_b, e->sel_q, e->CTXs, pt.R, Sp, H), false);
            auto norm_r = [&](const void* src, void* dst, const float* gamma) { return glc_launch_layernorm(st, dt, src, dst, gamma, e->zero_bias, c.ln_eps, pt.R, H); };
            if (!run_pruned_tail(e, pt, w, kGeGlu, H, norm_r)) return false; }                                                  // MB:299-476 on R rows
            return forward_epilogue(e, e->H1s, true, B, S, C, d_logits);
        }
        GemmArgs o;
        o.A = e->CTX; o.W = w.Wo; o.bias = nullptr; o.C = Xn; o.resid = X; o.Mpad = Mpad; o.N = H; o.K = H; o.gs_resid_plain = 1;
        if (mx) { o.W = w.Wo_x; o.mx_ws = w.ws_o; }
        { Prof p(e, PC_ATTN_OUT); KCHK(gs ? gemm_gs(EPI_RESID, o) : launch_gemm_auto(e, dt, EPI_RESID, o), false); }   // MB:299, :332
        std::swap(X, Xn);
        { Prof p(e, PC_LN); KCHK(norm(X, w.ln2), false); }                                                                  // MB:333
        GemmArgs f1;
        f1.A = e->H1; f1.W = w.Wgu; f1.bias = nullptr; f1.Mpad = Mpad; f1.N = 2 * I; f1.K = H;
        if (mx) { f1.W = w.Wgu_x; f1.mx_ws = w.ws_gu; f1.glu_interleaved = 1; }      // (mx implies fused_swiglu: Wi was interleaved at upload)
        if (!gated_ffn(e, kGeGlu, f1, gs, gemm_gs, M)) return false;                                                        // MB:89-91 gelu(input) * gate
        GemmArgs f2;
        f2.A = e->FF; f2.W = w.Wd; f2.bias = nullptr; f2.C = Xn; f2.resid = X; f2.Mpad = Mpad; f2.N = H; f2.K = I; f2.gs_resid_plain = 1;
        if (mx) { f2.W = w.Wd_x; f2.mx_ws = w.ws_d; }
        { Prof p(e, PC_FFN2); KCHK(gs ? gemm_gs(EPI_RESID, f2) : launch_gemm_auto(e, dt, EPI_RESID, f2), false); }
        std::swap(X, Xn);
        if (l + 1 < L && !dump_hidden(e, l + 1, X, M)) return false;
    }
    { Prof p(e, PC_LN); KCHK(glc_launch_layernorm(st, dt, X, e->H1, e->final_norm, e->zero_bias, c.ln_eps, M, H), false); }   // MB:476
    if (!dump_hidden(e, L, e->H1, M)) return false;
    return forward_epilogue(e, e->H1, false, B, S, C, d_logits);
}

// T5 / mT5 backbone (transformers 5.15 models/t5/modeling_t5.py, the encoder T5Stack, cited as T5:<line>): one launch sequence per batch.  The
// decoder's pre-norm residual stream on bias-free RMSNorms (T5LayerNorm, T5:50-71) and projections, without its norm fold and MX pipeline:
// x += O(Attn(RMS(x))) (T5LayerSelfAttention, T5:392-400), x += wo(gelu_new(wi_0 RMS(x)) * wi_1 RMS(x)) (T5LayerFF + T5DenseGatedActDense,
// T5:97-141), final_layer_norm behind the last block (T5:744).  The attention has no rotation (the layout pass gets cos = 1 / sin = 0), no
// 1/sqrt(d) scale (T5Attention.scaling = 1.0: qscale = log2(e) alone) and adds layer 0's relative-position bias, shared by every
// layer (T5:335-348, T5:738-740), ahead of the additive key mask: the RPB instantiations of the two attention kernels (decoder.hip).
// nh = t5_heads: cfg.heads rounded up to even, the extra head's weights zero (create_t5).  16-bit modes and the fp32 mode's small / odd
// shapes run plain rows of T; the fp32 mode runs the group-split pipeline under ModernBERT's conditions with the norms as kernels of their
// own.  The last layer is pruned as on the other pre-norm backbones (run_pruned_tail).  No MX pipeline.
bool run_forward_t5(glc_engine* e, const int64_t* ids, const int64_t* mask, int B, int S, int C, float* d_logits) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter, nh = e->t5_heads, d = c.head_dim, L = c.layers, NQ = nh * d;
    const int Sp = round_up(S, 64), M = B * Sp, Mpad = round_up(M, 256);
    hipStream_t st = e->stream;
    const int dt = e->dtype;
    if (!forward_prologue(e, ids, mask, B, S)) return false;
    void *X = e->X, *Xn = e->X2;
    { Prof p(e, PC_EMBED);                                                                                                  // T5:678 embed_tokens: no scale, no norm
      KCHK(glc_launch_embed_plain(st, dt, ids, mask, e->emb, X, e->kbias, B, S, Sp, H, c.vocab, c.pad_id), false); }
    if (!dump_hidden(e, 0, X, M)) return false;
    const float qscale = 1.4426950408889634f;                            // log2(e) for the exp2 softmax; T5 does not scale its scores
    const bool mfma = (dt != GLC_F32 || e->dec_split) && e->attn_impl != 1;
    bool gs = false;
    if (dt == GLC_F32 && e->gs_mode > 0 && e->w_presplit && e->dec_split && mfma && !e->keep_hidden && H % 256 == 0 && (2 * I) % 256 == 0 &&
        (3 * NQ) % 256 == 0 && NQ % 32 == 0 && I % 32 == 0) {
        GemmArgs t; t.Mpad = Mpad; t.N = H; t.K = H;
        gs = e->gs_mode == 2 || !glc_gemm_small_m(t);
    }
    e->last_gs = gs;
    e->last_lnf = false; e->last_mx = false; e->last_mx_attn = false; e->last_rope_epi = false; e->last_mx128 = 0; e->last_pruned = false;
    const GemmGs gemm_gs{st, false, M};
    const PrunedTail pt = pruned_tail(e, B, C);
    const float* cs = e->ropes[{Sp, 0.f}];
    const float* rpb = e->rpbs[Sp];
    auto norm = [&](const void* src, const float* gain) -> const char* {      // H1 = RMS(src) (group-split rows in the gs pipeline)
        return gs ? glc_launch_rmsnorm_gs(st, (const float*)src, e->H1, gain, c.ln_eps, M, H) : glc_launch_rmsnorm(st, dt, src, e->H1, gain, c.ln_eps, M, H);
    };
    for (int l = 0; l < L; ++l) {
        const DecLayerW& w = e->dlayers[l];
        const bool last = pt.on && l == L - 1;        // pruned (see run_pruned_tail): the residual rows the head reads, then K / V on every row
        const unsigned char* flag = last && mfma ? e->tile_flag : nullptr;
        if (last) {
            Prof p(e, PC_LAST);
            HIPCHK(hipMemsetAsync(e->tile_flag, 0, (size_t)Mpad >> 5, st), false);
            KCHK(glc_launch_gather_rows(st, dt, X, e->cls_pos, class_cap(e), e->Xs, e->sel_b, e->sel_q, e->tile_flag, B, Sp, H, pt.Cc, pt.klen), false);
        }
        { Prof p(e, last ? PC_LAST : PC_LN); KCHK(norm(X, w.ln1), false); }                                               // T5:392
        GemmArgs g;
        g.A = e->H1; g.W = w.Wqkv; g.bias = nullptr; g.C = e->QKV; g.Mpad = Mpad; g.N = 3 * NQ; g.K = H; g.gs_c_plain = 1;
        { Prof p(e, last ? PC_LAST : PC_QKV);
          KCHK(gs ? gemm_gs(EPI_BIAS, g) : launch_gemm_auto(e, dt, EPI_BIAS, g), false);                                    // T5:304-326 q / k / v
          if (mfma) KCHK(glc_launch_qkv_layout(st, dt, e->QKV, cs, e->Qh, e->Kh, e->Vt, B, Sp, nh, nh, d, qscale), false);
          else KCHK(glc_launch_rope_qk(st, dt, e->QKV, cs, M, Sp, nh, nh, d, qscale), false); }
        { Prof p(e, last ? PC_LAST : PC_ATTN);                                                                             // T5:335-364
          if (mfma) KCHK(glc_launch_attention_gqa_mfma(st, dt, e->Qh, e->Kh, e->Vt, e->kbias, e->klen, e->kfirst, e->CTX, B, Sp, nh, nh, d, 0, last ? 0 : (gs ? 1 : 0), 0, flag, rpb), false);
          else KCHK(glc_launch_attention_gqa(st, dt, 1, e->QKV, e->kbias, e->klen, e->CTX, B, Sp, nh, nh, d, 0, 0, rpb), false); }
        if (last) {
            { Prof p(e, PC_LAST);
            KCHK(glc_launch_gather_sel(st, dt, e->CTX, e->sel_b, e->sel_q, e->CTXs, pt.R, Sp, NQ), false);
            auto norm_r = [&](const void* src, void* dst, const float* gain) { return glc_launch_rmsnorm(st, dt, src, dst, gain, c.ln_eps, pt.R, H); };
            if (!run_pruned_tail(e, pt, w, kGeGluTanh, NQ, norm_r)) return false; }                                        // T5:367-744 on R rows
            return forward_epilogue(e, e->H1s, true, B, S, C, d_logits);
        }
        GemmArgs o;
        o.A = e->CTX; o.W = w.Wo; o.bias = nullptr; o.C = Xn; o.resid = X; o.Mpad = Mpad; o.N = H; o.K = NQ; o.gs_resid_plain = 1;
        { Prof p(e, PC_ATTN_OUT); KCHK(gs ? gemm_gs(EPI_RESID, o) : launch_gemm_auto(e, dt, EPI_RESID, o), false); }      // T5:367, :400
        std::swap(X, Xn);
        { Prof p(e, PC_LN); KCHK(norm(X, w.ln2), false); }                                                                 // T5:138
        GemmArgs f1;
        f1.A = e->H1; f1.W = w.Wgu; f1.bias = nullptr; f1.Mpad = Mpad; f1.N = 2 * I; f1.K = H;
        if (!gated_ffn(e, kGeGluTanh, f1, gs, gemm_gs, M)) return false;                                                   // T5:107-109 gelu_new(wi_0) * wi_1
        GemmArgs f2;
        f2.A = e->FF; f2.W = w.Wd; f2.bias = nullptr; f2.C = Xn; f2.resid = X; f2.Mpad = Mpad; f2.N = H; f2.K = I; f2.gs_resid_plain = 1;
        { Prof p(e, PC_FFN2); KCHK(gs ? gemm_gs(EPI_RESID, f2) : launch_gemm_auto(e, dt, EPI_RESID, f2), false); }        // T5:122, :140
        std::swap(X, Xn);
        if (l + 1 < L && !dump_hidden(e, l + 1, X, M)) return false;
    }
    { Prof p(e, PC_LN); KCHK(glc_launch_rmsnorm(st, dt, X, e->H1, e->final_norm, c.ln_eps, M, H), false); }                // T5:744
    if (!dump_hidden(e, L, e->H1, M)) return false;
    return forward_epilogue(e, e->H1, false, B, S, C, d_logits);
}

// BERT / RoBERTa / XLM-R backbone (transformers models/bert/modeling_bert.py): one launch sequence per batch.  Post-LayerNorm blocks as
// DeBERTa's, on the decoder's workspace and attention kernels: word + absolute position + token-type embedding under a LayerNorm (rows.hip
// embed_abs), then per layer QKV = x Wqkv^T + b, plain bidirectional attention (scores / sqrt(64), additive key mask; the layout pass with a
// table of cos = 1, sin = 0: no rotation), x = LN1(x + ctx Wo^T + bo), x = LN2(x + gelu_erf(x W1^T + b1) W2^T + b2).  No final norm.
// 16-bit modes and the fp32 mode's small / odd shapes run plain rows of T; the fp32 mode with H % 256 == 0 runs the group-split pipeline with
// the norms as kernels of their own (no fold): X, H1, CTX, FF as [32 hi | 32 lo] groups, the residual sums (X2) and QKV plain fp32.  No MX
// pipeline and no pruned last layer on this backbone.
bool run_forward_bert(glc_engine* e, const int64_t* ids, const int64_t* mask, int B, int S, int C, float* d_logits) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter, nh = c.heads, d = c.head_dim, L = c.layers;
    const int Sp = round_up(S, 64), M = B * Sp, Mpad = round_up(M, 256);
    hipStream_t st = e->stream;
    const int dt = e->dtype;
    if (!forward_prologue(e, ids, mask, B, S)) return false;
    const float qscale = 1.4426950408889634f / sqrtf((float)d);         // head_dim^-1/2, times log2(e) for the exp2 softmax
    const bool mfma = (dt != GLC_F32 || e->dec_split) && e->attn_impl != 1;
    bool gs = false;
    if (dt == GLC_F32 && e->gs_mode > 0 && e->w_presplit && e->dec_split && mfma && !e->keep_hidden && H % 256 == 0 && I % 256 == 0 && L > 0) {
        GemmArgs t; t.Mpad = Mpad; t.N = H; t.K = H;
        gs = e->gs_mode == 2 || !glc_gemm_small_m(t);
    }
    e->last_gs = gs;
    e->last_lnf = false; e->last_mx = false; e->last_mx_attn = false; e->last_rope_epi = false; e->last_mx128 = 0; e->last_pruned = false;
    const GemmGs gemm_gs{st, false, M};
    { Prof p(e, PC_EMBED);                                                                                   // BertEmbeddings.forward
      KCHK(glc_launch_pos_ids(st, ids, B, S, Sp, c.pad_id, c.pos_offset, e->pos_ids), false);
      if (gs) KCHK(glc_launch_embed_abs_gs(st, ids, mask, e->pos_ids, (const float*)e->emb, (const float*)e->pos_emb, (const float*)e->type_emb, e->eln_g, e->eln_b,
                                           c.ln_eps, e->X, e->kbias, B, S, Sp, H, c.vocab, c.pad_id, c.max_positions), false);
      else KCHK(glc_launch_embed_abs(st, dt, ids, mask, e->pos_ids, e->emb, e->pos_emb, e->type_emb, e->eln_g, e->eln_b, c.ln_eps, e->X, e->kbias, B, S, Sp, H,
                                     c.vocab, c.pad_id, c.max_positions), false); }
    if (!dump_hidden(e, 0, e->X, M)) return false;
    const float* cs = e->ropes[{Sp, 0.f}];
    void* T1 = e->X2;                         // the pre-norm sums (plain fp32 in the group-split pipeline)
    auto norm = [&](void* dst, const float* g, const float* b, bool plain) -> const char* {      // dst = LN(T1)
        return gs && !plain ? glc_launch_layernorm_gs(st, (const float*)T1, dst, g, b, c.ln_eps, M, H) : glc_launch_layernorm(st, dt, T1, dst, g, b, c.ln_eps, M, H);
    };
    for (int l = 0; l < L; ++l) {
        const LayerW& w = e->layers[l];
        GemmArgs g;
        g.A = e->X; g.W = w.Wqkv; g.bias = w.bqkv; g.C = e->QKV; g.Mpad = Mpad; g.N = 3 * H; g.K = H; g.gs_c_plain = 1;
        { Prof p(e, PC_QKV);
          KCHK(gs ? gemm_gs(EPI_BIAS, g) : launch_gemm_auto(e, dt, EPI_BIAS, g), false);                                   // BertSelfAttention query / key / value
          if (mfma) KCHK(glc_launch_qkv_layout(st, dt, e->QKV, cs, e->Qh, e->Kh, e->Vt, B, Sp, nh, nh, d, qscale), false);
          else KCHK(glc_launch_rope_qk(st, dt, e->QKV, cs, M, Sp, nh, nh, d, qscale), false); }
        { Prof p(e, PC_ATTN);
          if (mfma) KCHK(glc_launch_attention_gqa_mfma(st, dt, e->Qh, e->Kh, e->Vt, e->kbias, e->klen, e->kfirst, e->CTX, B, Sp, nh, nh, d, 0, gs ? 1 : 0, 0), false);
          else KCHK(glc_launch_attention_gqa(st, dt, 1, e->QKV, e->kbias, e->klen, e->CTX, B, Sp, nh, nh, d, 0), false); }
        GemmArgs o;
        o.A = e->CTX; o.W = w.Wo; o.bias = w.bo; o.C = T1; o.resid = e->X; o.Mpad = Mpad; o.N = H; o.K = H;
        { Prof p(e, PC_ATTN_OUT); KCHK(gs ? gemm_gs(EPI_RESID, o) : launch_gemm_auto(e, dt, EPI_RESID, o), false); }      // BertSelfOutput.dense + residual
        { Prof p(e, PC_LN); KCHK(norm(e->H1, w.ln1g, w.ln1b, false), false); }
        GemmArgs f1;
        f1.A = e->H1; f1.W = w.W1; f1.bias = w.b1; f1.C = e->FF; f1.Mpad = Mpad; f1.N = I; f1.K = H;
        { Prof p(e, PC_FFN1); KCHK(gs ? gemm_gs(EPI_GELU, f1) : launch_gemm_auto(e, dt, EPI_GELU, f1), false); }         // BertIntermediate
        GemmArgs f2;
        f2.A = e->FF; f2.W = w.W2; f2.bias = w.b2; f2.C = T1; f2.resid = e->H1; f2.Mpad = Mpad; f2.N = H; f2.K = I;
        { Prof p(e, PC_FFN2); KCHK(gs ? gemm_gs(EPI_RESID, f2) : launch_gemm_auto(e, dt, EPI_RESID, f2), false); }       // BertOutput.dense + residual
        // (the last layer's rows leave the group-split pipeline: the head reads plain fp32 rows)
        { Prof p(e, PC_LN); KCHK(norm(e->X, w.ln2g, w.ln2b, l == L - 1), false); }
        if (!dump_hidden(e, l + 1, e->X, M)) return false;
    }
    return forward_epilogue(e, e->X, false, B, S, C, d_logits);
}

// DeBERTa-v3 backbone: one launch sequence per batch (post-norm encoder with disentangled relative-position attention).
bool run_forward_deberta(glc_engine* e, const int64_t* ids, const int64_t* mask, int B, int S, int C, float* d_logits) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter, nh = c.heads;
    const int Sp = round_up(S, 64), M = B * Sp, Mpad = round_up(M, 256);
    hipStream_t st = e->stream;
    const int dt = e->dtype;
    const int ccap = class_cap(e);
    GxScope gx_scope(e);                     // fp8 range guard + activation exponent (see run_forward_decoder)
    if (!forward_prologue(e, ids, mask, B, S)) return false;
    // attention kernel: 3 = workgroup-shared band kernel (attention_wg.hip), 2 = per-wave band kernel (every operand type; fp32 native:
    // 32x32x2 MFMAs), 1 = straightforward kernel.  Default, measured same-box at c3 (scripts/attn_bench.py): split-f16 units of the
    // fp32 mode -> 3 (1.45 vs 1.80 ms per launch: MFMA-heavy, the 3 shared p2c MFMA blocks and the shared K / V^T ring pay);
    // 16-bit operands -> 2 (0.70 vs 0.76 ms: at one MFMA per product the kernel is bound by instruction issue and latency, and
    // the workgroup barrier per tile costs more than the 3 MFMAs and 3 loads it saves).  GLC_ATTN_WG=1 / 0 forces one or the other.
    static const int wg_env = glc_dev_env("GLC_ATTN_WG") ? atoi(glc_dev_env("GLC_ATTN_WG")) : -1;      // developer A/B switch
    const bool wg_pick = wg_env >= 0 ? wg_env != 0 : dt == GLC_F32;
    int impl = e->attn_impl ? e->attn_impl : ((wg_pick && (dt != GLC_F32 || e->attn_split)) ? 3 : 2);
    if (impl == 3 && dt == GLC_F32 && !e->attn_split) impl = 2;
    const bool asplit = e->attn_split && impl >= 2 && dt == GLC_F32;        // fp32 mode: split-f16 operand units for the band kernels
    auto launch_band = [&](const AttnArgs& aa) -> const char* {
        return impl == 3 ? glc_launch_attention_wg(st, dt, aa) : glc_launch_attention(st, dt, impl, aa);
    };
    const bool prune = e->prune_last && !e->keep_hidden && c.pooling == GLC_POOL_FIRST;
    e->last_pruned = false;
    // Group-split pipeline of the fp32 mode: the activations that feed GEMMs (X, H1, FF, CTX) are kept as [32 hi | 32 lo] f16 groups
    // (same bytes as fp32), written by their producers, so that every projection runs on the 256-tile LDS-DMA kernel with three
    // f16 MFMAs per product (gemm256s.hip, GS).  Needs the split-f16 weights and attention, the pruned last layer (its compact rows go back to plain
    // fp32 and the small-M kernels) and shapes the 256-tile kernel takes; small forwards stay on the 128-tile split-K kernels.
    bool gs = false, via_small = false;
    if (dt == GLC_F32 && e->gs_mode > 0 && e->w_presplit && asplit && impl == 3 && prune && H % 256 == 0 && I % 256 == 0) {
        GemmArgs t; t.Mpad = Mpad; t.N = H; t.K = H;
        gs = e->gs_mode == 2 || !glc_gemm_small_m(t);
        // opt-in (glc_engine_set_mx_small_forwards): a forward that fails only the fill rule of the 256 tile is still admitted, for the MX pipeline
        // alone — mode 1: when 128-tiles fill the device by the same rule, mode 2: always
        if (!gs && e->mx_small > 0 && (e->mx_small == 2 || (long long)(Mpad / 128) * (H / 128) * 2 >= glc_device_cus())) gs = via_small = true;
    }
    // MX pipeline (round 3): the group-split pipeline with GX rows and the MX cross-term GEMM (gemm256x.hip) for every projection of the
    // full layers — a_hi*w_hi as f16 MFMAs, both cross terms as one block-scaled fp8 MFMA.  Needs the LayerNorm fold on every layer.
    bool mx = gs && e->mx && e->mx_built && e->ln_fused && e->prec_mask == 0 && c.layers >= 2;
    for (int l = 0; mx && l < c.layers; ++l) mx = e->layers[l].W1f && (l == 0 || e->layers[l].Wqkvf);       // (the folded split-f16 copies the GX copies are made from)
    if (mx && !build_mx_weights(e)) mx = false;          // (no copies: this and every later forward stay on the split-f16 kernels)
    for (int l = 0; mx && l < c.layers; ++l) mx = e->layers[l].W1f_x && e->layers[l].Wqkv_x && e->layers[l].Wo_x && e->layers[l].W2_x && (l == 0 || e->layers[l].Wqkvf_x);
    if (via_small && !mx) gs = false;                    // (admitted for the MX pipeline only: without it the forward runs as it always has)
    e->last_gs = gs;
    e->last_mx = mx;
    e->last_mx_attn = false;
    e->last_mx128 = 0;
    const GemmGs gemm_gs{st, mx, M, mx ? e->mx_small : 0, &e->last_mx128};
    // 16-bit modes: the same LayerNorm fold on plain rows of T, when all four projections of a layer run on the staggered 256-tile kernel
    bool fold16 = false;
    if (dt != GLC_F32 && e->ln_fused && prune && !e->keep_hidden && e->attn_impl != 1 && H % 256 == 0 && I % 256 == 0 && e->statsA && e->statsB && e->ln_part) {
        GemmArgs t; t.Mpad = Mpad; t.N = H; t.K = H;
        fold16 = glc_gemm256_supported(dt, t) && !glc_gemm_small_m(t);
    }
    { Prof p(e, PC_EMBED);
      if (gs) KCHK(glc_launch_embed_gs(st, ids, mask, (const float*)e->emb, e->eln_g, e->eln_b, c.ln_eps, e->X, e->kbias, B, S, Sp, H, c.vocab, c.pad_id, mx ? 1 : 0), false);
      else KCHK(glc_launch_embed(st, dt, ids, mask, e->emb, e->eln_g, e->eln_b, c.ln_eps, e->X, e->kbias, B, S, Sp, H, c.vocab, c.pad_id), false); }
    if (!dump_hidden(e, 0, e->X, M)) return false;

    bool x_is_raw = false;
    for (int l = 0; l < c.layers; ++l) {
        const LayerW& w = e->layers[l];
        const bool last = prune && l == c.layers - 1;
        // LayerNorm folded away (group-split pipeline, e->ln_fused): X / H1 then hold the RAW residual sums of the producer GEMMs plus
        // (mean, rstd) per row in statsA / statsB; the consumers run on weights with gamma folded in.  Normalised rows stay where a
        // kernel outside the pipeline reads them: the embedding output (layer 0) and the input of the pruned last layer.
        const bool lnf = (gs || fold16) && e->ln_fused && w.W1f && (l == 0 || w.Wqkvf);
        if (l == 0) e->last_lnf = lnf;
        const bool x_raw = x_is_raw;         // X holds raw sums + statsA (written by the previous layer's FFN2)
        GemmArgs g;
        g.A = e->X; g.W = w.Wqkv; g.bias = w.bqkv; g.Qh = e->Qh; g.Kh = e->Kh; g.Vt = e->Vt;
        g.Mpad = Mpad; g.N = 3 * H; g.K = H; g.Mvalid = M; g.Sp = Sp; g.nh = nh; g.H = H; g.qkv_split = asplit;
        if (last) break;
        if (x_raw) { g.W = w.Wqkvf; g.bias = w.dq; g.a_stats = e->statsA; g.ln_c = w.cq; }
        const bool mxa = mx && e->mx_attn && w.PKm && w.PQm;       // attention of this layer on MX tiles
        if (mx) { g.W = x_raw ? w.Wqkvf_x : w.Wqkv_x; g.mx_ws = x_raw ? w.ws_qkvf : w.ws_qkv; g.qkv_mxt = mxa ? 1 : 0; }
        const int pm = gs ? e->prec_mask : 0;
        g.prec = pm & 3;
        { Prof p(e, PC_QKV); KCHK(gs ? gemm_gs(EPI_QKV, g) : launch_gemm_auto(e, dt, EPI_QKV, g), false); }
        if (e->debug_stop >= 10 * l && e->debug_stop <= 10 * l + 4) { e->lastB = B; e->lastS = S; e->lastSp = Sp; }      // (a stopped forward still describes the workspace it leaves)
        if (e->debug_stop == 10 * l + 0) return true;
        AttnArgs a{e->Qh, e->Kh, e->Vt, asplit ? w.PKs : w.PK, asplit ? w.PQs : w.PQ, e->dtabs[Sp], e->kbias, e->klen, e->kfirst, e->CTX, B, nh, Sp, H, e->P};
        a.split = asplit; a.ctx_gs = mx ? 2 : (gs ? 1 : 0); a.prec = (pm >> 8) & 63;
        static const bool nosat = glc_dev_env("GLC_ATTN_NOSAT") != nullptr;      // A/B switch (developer)
        if (!nosat) { a.rsat_pos = e->dsat[Sp].first; a.rsat_neg = e->dsat[Sp].second; }
        a.otab = e->otabs[Sp]; a.mtab = e->mtabs.count(Sp) ? e->mtabs[Sp] : nullptr;
        if (mxa) { a.PK = w.PKm; a.PQ = w.PQm; e->last_mx_attn = true; }
        { Prof p(e, PC_ATTN); KCHK(mxa ? glc_launch_attention_mx(st, a) : launch_band(a), false); }
        if (e->debug_stop == 10 * l + 1) return true;
        GemmArgs o;
        o.A = e->CTX; o.W = w.Wo; o.bias = w.bo; o.C = e->T1; o.resid = e->X; o.Mpad = Mpad; o.N = H; o.K = H;
        if (x_raw) { const LayerW& wp = e->layers[l - 1]; o.r_stats = e->statsA; o.r_gamma = wp.ln2g; o.r_beta = wp.ln2b; }
        if (lnf) { o.C = e->H1; o.ln_part = e->ln_part; }      // raw sum -> H1 (group-split rows) + partials
        o.prec = ((pm >> 2) & 3) | ((pm & PM_RESID) ? 4 : 0);
        if (mx) { o.W = w.Wo_x; o.mx_ws = w.ws_o; }
        { Prof p(e, PC_ATTN_OUT); KCHK(gs ? gemm_gs(EPI_RESID, o) : launch_gemm_auto(e, dt, EPI_RESID, o), false); }
        { Prof p(e, PC_LN); KCHK(lnf ? glc_launch_ln_stats(st, e->ln_part, H / 64, e->statsB, M, H, c.ln_eps)
                                 : gs ? glc_launch_layernorm_gs(st, (const float*)e->T1, e->H1, w.ln1g, w.ln1b, c.ln_eps, M, H)
                                      : glc_launch_layernorm(st, dt, e->T1, e->H1, w.ln1g, w.ln1b, c.ln_eps, M, H), false); }
        if (e->debug_stop == 10 * l + 2) return true;
        GemmArgs f1;
        f1.A = e->H1; f1.W = w.W1; f1.bias = w.b1; f1.C = e->FF; f1.Mpad = Mpad; f1.N = I; f1.K = H;
        if (lnf) { f1.W = w.W1f; f1.bias = w.d1; f1.a_stats = e->statsB; f1.ln_c = w.c1; }
        f1.prec = (pm >> 4) & 3;
        if (mx) { f1.W = w.W1f_x; f1.mx_ws = w.ws_1f; }
        { Prof p(e, PC_FFN1); KCHK(gs ? gemm_gs(EPI_GELU, f1) : launch_gemm_auto(e, dt, EPI_GELU, f1), false); }
        if (e->debug_stop == 10 * l + 3) return true;
        GemmArgs f2;
        f2.A = e->FF; f2.W = w.W2; f2.bias = w.b2; f2.C = e->T1; f2.resid = e->H1; f2.Mpad = Mpad; f2.N = H; f2.K = I;
        if (lnf) { f2.r_stats = e->statsB; f2.r_gamma = w.ln1g; f2.r_beta = w.ln1b; }
        f2.prec = ((pm >> 6) & 3) | ((pm & PM_RESID) ? 4 : 0);
        // the next consumer of X takes raw rows only if it is a folded QKV of the pipeline (not the pruned last layer, which gathers normalised rows)
        const bool next_raw = lnf && l + 1 < c.layers && e->layers[l + 1].Wqkvf && !(prune && l + 1 == c.layers - 1);
        if (next_raw) { f2.C = e->X; f2.ln_part = e->ln_part; }
        if (mx) { f2.W = w.W2_x; f2.mx_ws = w.ws_2; }
        { Prof p(e, PC_FFN2); KCHK(gs ? gemm_gs(EPI_RESID, f2) : launch_gemm_auto(e, dt, EPI_RESID, f2), false); }
        { Prof p(e, PC_LN); KCHK(next_raw ? glc_launch_ln_stats(st, e->ln_part, H / 64, e->statsA, M, H, c.ln_eps)
                                 : gs ? glc_launch_layernorm_gs(st, (const float*)e->T1, e->X, w.ln2g, w.ln2b, c.ln_eps, M, H, mx ? 1 : 0)
                                      : glc_launch_layernorm(st, dt, e->T1, e->X, w.ln2g, w.ln2b, c.ln_eps, M, H), false); }
        x_is_raw = next_raw;
        if (e->debug_stop == 10 * l + 4) return true;
        if (!dump_hidden(e, l + 1, e->X, M)) return false;
    }
    const int Cc = class_rows(e, C);
    if (prune) {
        // Last layer, exact pruning: the head reads only the [CLS] row and the class-token rows, so only those
        // R = B*(1+C) rows need Q, attention output, the output projection and the FFN.  K and V^T are still
        // produced for every position (they are what the selected queries attend to).
        Prof p(e, PC_LAST);
        const LayerW& w = e->layers[c.layers - 1];
        const int R = B * (1 + Cc), Rpad = round_up(R, 256);
        const bool band_sel = impl >= 2;     // band kernel on the query tiles that hold selected rows; impl 1: row-selection kernel
        GemmArgs g;
        g.A = e->X; g.W = w.Wqkv; g.bias = w.bqkv; g.Qh = e->Qh; g.Kh = e->Kh; g.Vt = e->Vt; g.qkv_skip_q = band_sel ? 0 : 1;
        g.Mpad = Mpad; g.N = 3 * H; g.K = H; g.Mvalid = M; g.Sp = Sp; g.nh = nh; g.H = H; g.qkv_split = asplit && band_sel;
        if (band_sel) HIPCHK(hipMemsetAsync(e->tile_flag, 0, (size_t)Mpad >> 5, st), false);
        // (group-split pipeline: the compact rows leave it here — plain fp32, the rest of this layer runs on the small-M kernels)
        if (gs) KCHK(glc_launch_gather_rows_gs(st, e->X, e->cls_pos, ccap, (float*)e->Xs, e->sel_b, e->sel_q, band_sel ? e->tile_flag : nullptr, B, Sp, H, Cc, mx ? 1 : 0), false);
        else KCHK(glc_launch_gather_rows(st, dt, e->X, e->cls_pos, ccap, e->Xs, e->sel_b, e->sel_q, band_sel ? e->tile_flag : nullptr, B, Sp, H, Cc), false);
        if (gs) g.prec = e->prec_mask & 3;
        if (mx) { g.W = w.Wqkv_x; g.mx_ws = w.ws_qkv; }
        if (band_sel) g.q_tile_flag = e->tile_flag;       // the gather has flagged the query tiles that hold selected rows: the Q third skips the others
        KCHK(gs ? gemm_gs(EPI_QKV, g) : launch_gemm_auto(e, dt, EPI_QKV, g), false);
        if (band_sel) {
            AttnArgs a{e->Qh, e->Kh, e->Vt, asplit ? w.PKs : w.PK, asplit ? w.PQs : w.PQ, e->dtabs[Sp], e->kbias, e->klen, e->kfirst, e->CTX, B, nh, Sp, H, e->P};
            a.rsat_pos = e->dsat[Sp].first; a.rsat_neg = e->dsat[Sp].second; a.tile_flag = e->tile_flag; a.otab = e->otabs[Sp]; a.split = asplit;
            // selected query tiles only: the per-wave kernel skips every other tile; a workgroup of the shared kernel would run all
            // its waves for the one tile that holds the [CLS] / class-token rows
            static const bool ksplit_on = !(glc_dev_env("GLC_ATTN_KSPLIT") && atoi(glc_dev_env("GLC_ATTN_KSPLIT")) == 0);     // developer A/B switch
            a.ksplit = ksplit_on ? 1 : 0;       // a workgroup with one selected query tile splits that tile's keys over its four waves
            KCHK(e->attn_impl == 3 ? launch_band(a) : glc_launch_attention(st, dt, 2, a), false);
            KCHK(glc_launch_gather_sel(st, dt, e->CTX, e->sel_b, e->sel_q, e->CTXs, R, Sp, H), false);
        } else {
            GemmArgs gq;     // Q rows of the selection: the first H rows of the fused [3H,H] weight are the (pre-scaled) query projection
            gq.A = e->Xs; gq.W = w.Wqkv; gq.bias = w.bqkv; gq.C = e->Qs; gq.Mpad = Rpad; gq.N = H; gq.K = H;
            KCHK(launch_gemm_auto(e, dt, EPI_BIAS, gq), false);
            AttnArgs a{nullptr, e->Kh, e->Vt, w.PK, w.PQ, e->dtabs[Sp], e->kbias, e->klen, e->kfirst, e->CTXs, B, nh, Sp, H, e->P};
            a.sel_b = e->sel_b; a.sel_q = e->sel_q; a.Qrow = e->Qs; a.nsel = R;
            KCHK(glc_launch_attention(st, dt, 1, a), false);
        }
        GemmArgs o;
        o.A = e->CTXs; o.W = w.Wo; o.bias = w.bo; o.C = e->T1s; o.resid = e->Xs; o.Mpad = Rpad; o.N = H; o.K = H;
        KCHK(launch_gemm_auto(e, dt, EPI_RESID, o), false);
        KCHK(glc_launch_layernorm(st, dt, e->T1s, e->H1s, w.ln1g, w.ln1b, c.ln_eps, R, H), false);
        GemmArgs f1;
        f1.A = e->H1s; f1.W = w.W1; f1.bias = w.b1; f1.C = e->FFs; f1.Mpad = Rpad; f1.N = I; f1.K = H;
        KCHK(launch_gemm_auto(e, dt, EPI_GELU, f1), false);
        GemmArgs f2;
        f2.A = e->FFs; f2.W = w.W2; f2.bias = w.b2; f2.C = e->T1s; f2.resid = e->H1s; f2.Mpad = Rpad; f2.N = H; f2.K = I;
        KCHK(launch_gemm_auto(e, dt, EPI_RESID, f2), false);
        KCHK(glc_launch_layernorm(st, dt, e->T1s, e->Xs, w.ln2g, w.ln2b, c.ln_eps, R, H), false);
    }
    e->last_pruned = prune;
    return forward_epilogue(e, prune ? e->Xs : e->X, prune, B, S, C, d_logits);
}

// The launch sequence for one batch.  ids/mask are device pointers.
bool run_forward(glc_engine* e, const int64_t* ids, const int64_t* mask, int B, int S, int C, float* d_logits) {
    switch (e->cfg.backbone) {
    case GLC_BACKBONE_DECODER: return run_forward_decoder(e, ids, mask, B, S, C, d_logits);
    case GLC_BACKBONE_MODERNBERT: return run_forward_modernbert(e, ids, mask, B, S, C, d_logits);
    case GLC_BACKBONE_BERT: return run_forward_bert(e, ids, mask, B, S, C, d_logits);
    case GLC_BACKBONE_T5: return run_forward_t5(e, ids, mask, B, S, C, d_logits);
    default: return run_forward_deberta(e, ids, mask, B, S, C, d_logits);
    }
}

// Captured-graph replay (opt-in, glc_engine_set_graph_replay).  A forward of a few rows is a hundred and more launches of a few
// microseconds each; replay makes their submission one call for a caller that sends the same shapes again and again (measured: no throughput
// gain with the stream kept full — the device's time per launch bounds such a forward, profiles/graph_replay/summary.txt).  Per key
// (GraphKey: shape, pipeline switches, workspace generation, the three device pointers): the FIRST forward runs eagerly — it has sized the
// workspace, built the tables and the MX weights, raised the LDS limits and allocated the gated FFN's rows before it returns —, the SECOND
// is captured on the engine's one stream (a linear chain: no forks, no events), instantiated and launched, every later one is one
// hipGraphLaunch.  The captured region is run_forward alone: kernel launches, device-to-device copies and memsets on buffers whose
// addresses the key pins.  H2D / D2H copies of the host-buffer entry, the range guard's counter read and every host decision stay outside.
GraphKey graph_key(const glc_engine* e, const void* ids, const void* mask, int B, int S, int C, const void* d_logits) {
    GraphKey k;
    k.backbone = e->cfg.backbone; k.head = e->cfg.head_kind; k.B = B; k.S = S; k.Sp = round_up(S, 64); k.C = C;
    k.gs_mode = e->gs_mode; k.mx = e->mx && e->mx_built ? 1 : 0; k.mx_attn = e->mx_attn ? 1 : 0; k.ln_fused = e->ln_fused ? 1 : 0;
    k.prune = e->prune_last ? 1 : 0; k.attn_impl = e->attn_impl; k.prec_mask = e->prec_mask; k.act_sc = e->act_sc; k.sticky = e->fp8_sticky_off ? 1 : 0;
    k.full_lines = glc_gemm_full_lines(); k.mx_small = e->mx_small;
    k.ws_gen = e->ws_gen; k.ids = ids; k.mask = mask; k.logits = d_logits;
    return k;
}
GraphEntry* graph_find(glc_engine* e, const GraphKey& k) {
    for (GraphEntry& g : e->graphs) if (g.key == k) return &g;
    return nullptr;
}
int graph_count(const glc_engine* e) {
    int n = 0;
    for (const GraphEntry& g : e->graphs) n += g.exec ? 1 : 0;
    return n;
}
// drop the least recently used entry (execs_only: among those that hold an executable)
void graph_evict(glc_engine* e, bool execs_only) {
    int lru = -1;
    for (size_t i = 0; i < e->graphs.size(); ++i)
        if ((!execs_only || e->graphs[i].exec) && (lru < 0 || e->graphs[i].tick < e->graphs[lru].tick)) lru = (int)i;
    if (lru < 0) return;
    if (e->graphs[lru].exec) { (void)hipStreamSynchronize(e->stream); (void)hipGraphExecDestroy(e->graphs[lru].exec); }
    e->graphs.erase(e->graphs.begin() + lru);
}
void graph_note_last(const glc_engine* e, GraphEntry& g) {
    g.gs = e->last_gs; g.lnf = e->last_lnf; g.mx = e->last_mx; g.mx_attn = e->last_mx_attn; g.rope_epi = e->last_rope_epi; g.pruned = e->last_pruned;
    g.mx128 = e->last_mx128;
}

// run_forward, or its captured graph.  Sets e->last_graph.  Caller holds e->mu and has called ensure_capacity.
bool graph_forward(glc_engine* e, const int64_t* ids, const int64_t* mask, int B, int S, int C, float* d_logits) {
    e->last_graph = 0;
    // event bracketing, the hidden-state dump and a stopped forward are not replayed
    if (!e->graph_on || e->profile || e->keep_hidden || e->debug_stop >= 0) return run_forward(e, ids, mask, B, S, C, d_logits);
    const GraphKey key = graph_key(e, ids, mask, B, S, C, d_logits);
    GraphEntry* g = graph_find(e, key);
    if (g && g->exec) {
        if (hipGraphLaunch(g->exec, e->stream) == hipSuccess) {
            g->tick = ++e->graph_tick;
            e->last_gs = g->gs; e->last_lnf = g->lnf; e->last_mx = g->mx; e->last_mx_attn = g->mx_attn; e->last_rope_epi = g->rope_epi; e->last_pruned = g->pruned; e->last_mx128 = g->mx128;
            e->lastB = B; e->lastS = S; e->lastSp = key.Sp;
            e->last_graph = 2;
            return true;
        }
        (void)hipGetLastError();            // (refused: nothing was enqueued — this key runs eagerly from now on)
        (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; g->ineligible = true;
        return run_forward(e, ids, mask, B, S, C, d_logits);
    }
    if (g && !g->ineligible) {
        // second forward of the key: capture.  Thread-local mode: a session runs one host thread per engine, and another thread's hipMalloc
        // must not invalidate this capture.  Whatever goes wrong — a launcher that refuses, an allocation (dmalloc refuses while capturing),
        // an error from the runtime — ends the capture, destroys what was recorded and runs the forward eagerly: nothing half-captured runs.
        g->tick = ++e->graph_tick;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            e->capturing = true;
            const bool ok = run_forward(e, ids, mask, B, S, C, d_logits);
            e->capturing = false;
            const hipError_t ce = hipStreamEndCapture(e->stream, &graph);
            if (ok && ce == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) exec = nullptr;
            if (graph) (void)hipGraphDestroy(graph);
            if (!ok || ce != hipSuccess) exec = nullptr;
        }
        if (exec) {
            if (graph_count(e) >= kGraphCacheMax) { graph_evict(e, true); g = graph_find(e, key); }
            if (g && hipGraphLaunch(exec, e->stream) == hipSuccess) {
                g->exec = exec;
                graph_note_last(e, *g);
                e->last_graph = 1;
                return true;
            }
            (void)hipGraphExecDestroy(exec);
        }
        (void)hipGetLastError();
        if ((g = graph_find(e, key))) g->ineligible = true;
        return run_forward(e, ids, mask, B, S, C, d_logits);
    }
    if (!run_forward(e, ids, mask, B, S, C, d_logits)) return false;
    if (!g) {
        // warmed up: the key as it reads NOW (the forward may have freed a buffer — the gated FFN's rows — or lost the MX pipeline)
        const GraphKey now = graph_key(e, ids, mask, B, S, C, d_logits);
        if (!graph_find(e, now)) {
            if ((int)e->graphs.size() >= kGraphKeysMax) graph_evict(e, false);
            GraphEntry n; n.key = now; n.tick = ++e->graph_tick;
            e->graphs.push_back(n);
        }
    }
    return true;
}

// the largest tensor (in floats) a backbone's loader sends through the staging buffer: the embedding, the fused QKV weight (the folded
// copy goes up in one piece) or the FFN's input weight (the gated FFNs' [first | second] rows in one piece)
size_t staging_floats(const glc_model_config& c) {
    const size_t H = c.hidden, I = c.inter;
    const size_t qkv = c.backbone == GLC_BACKBONE_DECODER ? (size_t)(c.heads + 2 * c.kv_heads) * c.head_dim
                     : c.backbone == GLC_BACKBONE_T5 ? 3 * (size_t)((c.heads + 1) / 2 * 2) * c.head_dim : 3 * H;
    const size_t ffn = c.backbone == GLC_BACKBONE_DEBERTA || c.backbone == GLC_BACKBONE_BERT ? I : 2 * I;
    const size_t pos = c.backbone == GLC_BACKBONE_BERT ? (size_t)c.max_positions : 0;
    return std::max({(size_t)c.vocab * H, qkv * H, ffn * H, pos * H});
}

// one projection weight: the slot of its device copy and its host row blocks, in order
struct Proj { void** dst; std::vector<std::pair<const float*, size_t>> parts; };
// A layer's projection weights: each allocated as T and uploaded from its row blocks, then (fp32 mode) split into group-split rows
// once — the operand image of both split-f16 GEMM kernels
bool upload_projections(glc_engine* e, float* staging, std::initializer_list<Proj> ws) {
    const size_t es = esize(e->dtype);
    for (const Proj& p : ws) {
        size_t n = 0;
        for (const auto& part : p.parts) n += part.second;
        *p.dst = dmalloc(e, n * es, false);
        if (!*p.dst) return false;
        size_t off = 0;
        for (const auto& part : p.parts) {
            if (!upload_as(e, part.first, part.second, (char*)*p.dst + off * es, staging)) return false;
            off += part.second;
        }
        if (e->w_presplit && e->dtype == GLC_F32) KCHK(glc_launch_presplit(e->stream, *p.dst, n), false);
    }
    return true;
}

// The weight rows of a gated FFN that runs its gate in the GEMM epilogue (fused_swiglu): rows [32 f, 32 f + 16) = the first half's rows of
// features 16 f .. 16 f + 15 (decoder gate, ModernBERT input), rows [32 f + 16, 32 f + 32) = the second half's rows of the same features
void interleave_glu_rows(const float* first, const float* second, int I, int H, std::vector<float>& dst) {
    dst.resize(2 * (size_t)I * H);
    for (int f = 0; f < I / 16; ++f) {
        memcpy(dst.data() + (size_t)(32 * f) * H, first + (size_t)(16 * f) * H, (size_t)16 * H * sizeof(float));
        memcpy(dst.data() + (size_t)(32 * f + 16) * H, second + (size_t)(16 * f) * H, (size_t)16 * H * sizeof(float));
    }
}

// The head (the last tensors of every backbone): the two FeaturesProjectors' 8 tensors and the scorer's, then the load's final sync
bool upload_head(glc_engine* e, const float* const* ht) {
    const size_t H = e->cfg.hidden;
    for (int i = 0; i < 8; ++i) {
        e->headw[i] = upload_f32(e, ht[i], i % 2 == 0 ? H * H : H);
        if (!e->headw[i]) return false;
        if (i % 2 == 0 && e->w_presplit) KCHK(glc_launch_presplit(e->stream, e->headw[i], H * H), false);
    }
    if (!upload_scorer(e, ht + GLC_TENSORS_HEAD)) return false;
    if (hipStreamSynchronize(e->stream) != hipSuccess) { glc_set_err(std::string("engine_create: ") + hipGetErrorString(hipGetLastError())); return false; }
    return true;
}

// The sequence-classification head's six slots (include/gliclass_hip.h; create has checked which may be null), then the load's final sync
bool upload_cls_head(glc_engine* e, const float* const* ht) {
    const size_t H = e->cfg.hidden, K = e->cfg.cls_labels;
    const size_t n[GLC_TENSORS_CLS_HEAD] = {H * H, H, H, H, K * H, K};
    for (int i = 0; i < GLC_TENSORS_CLS_HEAD; ++i) {
        if (!ht[i]) continue;
        e->clsw[i] = upload_f32(e, ht[i], n[i]);
        if (!e->clsw[i]) return false;
        if (i == 0 && e->w_presplit) KCHK(glc_launch_presplit(e->stream, e->clsw[0], H * H), false);
    }
    if (hipStreamSynchronize(e->stream) != hipSuccess) { glc_set_err(std::string("engine_create: ") + hipGetErrorString(hipGetLastError())); return false; }
    return true;
}

// Decoder backbone: upload + convert weights.  Fused operands: Wqkv = [q_proj; k_proj; v_proj] rows, Wgu = [gate_proj; up_proj]
// rows, so each layer runs four GEMMs (Q2:206-208 as one, Q2:233, Q2:47 gate|up as one, down).
bool create_decoder(glc_engine* e, const float* const* tensors, float* staging) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter, L = c.layers, d = c.head_dim;
    const size_t NQ = (size_t)c.heads * d, NKV = (size_t)c.kv_heads * d, NQKV = NQ + 2 * NKV, IH = (size_t)I * H;
    e->dlayers.resize(L);
    std::vector<float> bqkv(NQKV), gu_host, fold_host;
    const int per = glc_dec_tensors_per_layer(&c);
    for (int l = 0; l < L; ++l) {
        // the layer's tensors in the Qwen2 numbering whatever the model carries (include/gliclass_hip.h): ln1 qw qb kw kb vw vb ow ln2 gw uw dw,
        // then q_norm, k_norm; absent ones (the biases without attn_bias, the gains without qk_norm) stay null
        const float* t[14] = {nullptr};
        {
            const float* const* src = tensors + 1 + per * l;
            int j = 0;
            t[0] = src[j++];
            for (int k = 1; k <= 5; k += 2) { t[k] = src[j++]; if (c.attn_bias) t[k + 1] = src[j++]; }
            if (c.qk_norm) { t[12] = src[j++]; t[13] = src[j++]; }
            for (int k = 7; k <= 11; ++k) t[k] = src[j++];
        }
        DecLayerW& w = e->dlayers[l];
        if (e->fused_swiglu) interleave_glu_rows(t[9], t[10], I, H, gu_host);
        const Proj gu = e->fused_swiglu ? Proj{&w.Wgu, {{gu_host.data(), 2 * IH}}} : Proj{&w.Wgu, {{t[9], IH}, {t[10], IH}}};
        if (!upload_projections(e, staging, {{&w.Wqkv, {{t[1], NQ * H}, {t[3], NKV * H}, {t[5], NKV * H}}}, {&w.Wo, {{t[7], H * NQ}}}, gu, {&w.Wd, {{t[11], IH}}}}))
            return false;
        if (e->ln_fused && e->w_presplit && e->dtype == GLC_F32 && e->fused_swiglu && H % 64 == 0) {
            // RMSNorm folded into the consumer GEMMs of the group-split pipeline: RMSNorm(x) W^T = rstd (x (W diag(gamma))^T)
            auto fold_rows = [&](const float* Wsrc, size_t rows, const float* gam, float* dst) {
                for (size_t n = 0; n < rows; ++n) for (int k = 0; k < H; ++k) dst[n * H + k] = Wsrc[n * H + k] * gam[k];
            };
            std::vector<float>& wf = fold_host;
            wf.resize(2 * IH > NQKV * H ? 2 * IH : NQKV * H);
            fold_rows(t[1], NQ, t[0], wf.data()); fold_rows(t[3], NKV, t[0], wf.data() + NQ * H); fold_rows(t[5], NKV, t[0], wf.data() + (NQ + NKV) * H);
            if (!upload_projections(e, staging, {{&w.Wqkvf, {{wf.data(), NQKV * H}}}})) return false;
            fold_rows(gu_host.data(), 2 * (size_t)I, t[8], wf.data());           // the interleaved [16 gate | 16 up] row order is kept
            if (!upload_projections(e, staging, {{&w.Wguf, {{wf.data(), 2 * IH}}}})) return false;
        }
        if (c.attn_bias) {
            for (size_t i = 0; i < NQ; ++i) bqkv[i] = t[2][i];
            for (size_t i = 0; i < NKV; ++i) { bqkv[NQ + i] = t[4][i]; bqkv[NQ + NKV + i] = t[6][i]; }
            w.bqkv = upload_f32(e, bqkv.data(), NQKV);
            if (!w.bqkv) return false;
        }
        if (c.qk_norm) {
            w.qn = upload_f32(e, t[12], d); w.kn = upload_f32(e, t[13], d);
            if (!w.qn || !w.kn) return false;
        }
        w.ln1 = upload_f32(e, t[0], H); w.ln2 = upload_f32(e, t[8], H);
        if (!w.ln1 || !w.ln2) return false;
        if (hipStreamSynchronize(e->stream) != hipSuccess) { glc_set_err("sync failed"); return false; }   // bqkv host buffer is reused
    }
    e->final_norm = upload_f32(e, tensors[1 + per * L], H);
    return e->final_norm != nullptr;
}

// ModernBERT backbone: upload + convert weights (include/gliclass_hip.h tensor order).  Per layer: Wqkv as it is (rows Q | K | V), Wo,
// Wi (rows input | gate; interleaved 16 input / 16 gate rows when GeGLU runs in the GEMM epilogue, as the decoder's gate / up), mlp.Wo.
bool create_modernbert(glc_engine* e, const float* const* tensors, float* staging) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter, L = c.layers;
    const size_t HH = (size_t)H * H, IH = (size_t)I * H;
    e->eln_g = upload_f32(e, tensors[1], H);
    e->zero_bias = (float*)dmalloc(e, (size_t)H * sizeof(float));
    if (!e->eln_g || !e->zero_bias) return false;
    e->dlayers.resize(L);
    std::vector<float> wi_host;
    for (int l = 0; l < L; ++l) {
        const float* const* t = tensors + glc_mb_layer_base(l);
        const float* attn_norm = l > 0 ? t[0] : nullptr;
        if (l > 0) ++t;                                          // t: Wqkv Wo mlp_norm Wi Wo
        DecLayerW& w = e->dlayers[l];
        if (e->fused_swiglu) interleave_glu_rows(t[3], t[3] + IH, I, H, wi_host);
        if (!upload_projections(e, staging, {{&w.Wqkv, {{t[0], 3 * HH}}}, {&w.Wo, {{t[1], HH}}}, {&w.Wgu, {{e->fused_swiglu ? wi_host.data() : t[3], 2 * IH}}},
                                             {&w.Wd, {{t[4], IH}}}}))
            return false;
        if (attn_norm && !(w.ln1 = upload_f32(e, attn_norm, H))) return false;
        if (!(w.ln2 = upload_f32(e, t[2], H))) return false;
        // (the largest element a normalised row can hold, |gamma| sqrt(H): the rows of these norms are GX operands on the MX pipeline, glc_engine_enable_mx)
        for (int i = 0; i < H; ++i) e->mb_ln_bound = fmaxf(e->mb_ln_bound, fmaxf(attn_norm ? fabsf(attn_norm[i]) : fabsf(tensors[1][i]), fabsf(t[2][i])) * sqrtf((float)H));
    }
    e->final_norm = upload_f32(e, tensors[L > 0 ? glc_mb_layer_base(L) : 2], H);
    return e->final_norm != nullptr;
}

// T5 backbone: upload + convert weights (include/gliclass_hip.h tensor order).  rel_bias stays on the host (build_rpb_table turns it into
// one device table per padded length).  Per layer the fused Wqkv (rows q | k | v), o, the fused [wi_0 | wi_1] and wo as they come — except
// with an odd head count: the kernels run t5_heads = heads + 1 heads, so q, k and v each get 64 zero rows behind their own and o 64 zero
// columns (the extra head attends uniformly over zero values and multiplies zero weights: it adds exactly 0).
bool create_t5(glc_engine* e, const float* const* tensors, float* staging) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter, L = c.layers, d = c.head_dim;
    const size_t IN = (size_t)c.heads * d, NQ = (size_t)e->t5_heads * d, IH = (size_t)I * H;
    e->rel_bias.assign(tensors[1], tensors[1] + (size_t)c.rel_buckets * c.heads);
    e->dlayers.resize(L);
    std::vector<float> qkv_host, o_host;
    for (int l = 0; l < L; ++l) {
        const float* const* t = tensors + GLC_T5_TENSORS_FIXED + GLC_T5_TENSORS_PER_LAYER * l;      // t: ln1 Wqkv Wo ln2 Wgu Wd
        DecLayerW& w = e->dlayers[l];
        const float *wqkv = t[1], *wo = t[2];
        if (NQ != IN) {
            qkv_host.assign(3 * NQ * H, 0.f); o_host.assign((size_t)H * NQ, 0.f);
            for (int p = 0; p < 3; ++p) memcpy(qkv_host.data() + p * NQ * H, t[1] + p * IN * H, IN * H * sizeof(float));
            for (int r = 0; r < H; ++r) memcpy(o_host.data() + r * NQ, t[2] + r * IN, IN * sizeof(float));
            wqkv = qkv_host.data(); wo = o_host.data();
        }
        if (!upload_projections(e, staging, {{&w.Wqkv, {{wqkv, 3 * NQ * H}}}, {&w.Wo, {{wo, (size_t)H * NQ}}}, {&w.Wgu, {{t[4], 2 * IH}}}, {&w.Wd, {{t[5], IH}}}})) return false;
        w.ln1 = upload_f32(e, t[0], H); w.ln2 = upload_f32(e, t[3], H);
        if (!w.ln1 || !w.ln2) return false;
        if (hipStreamSynchronize(e->stream) != hipSuccess) { glc_set_err("sync failed"); return false; }   // the padded host buffers are reused
    }
    e->final_norm = upload_f32(e, tensors[GLC_T5_TENSORS_FIXED + GLC_T5_TENSORS_PER_LAYER * L], H);
    return e->final_norm != nullptr;
}

// BERT / RoBERTa / XLM-R backbone: upload + convert weights (include/gliclass_hip.h tensor order).  The position table and row 0 of the
// token-type table (the only row a forward uses: the reference passes no token types) as T beside the word table; per layer the fused
// Wqkv / bqkv as they come, Wo, W1, W2 with their biases and the two LayerNorms.
bool create_bert(glc_engine* e, const float* const* tensors, float* staging) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter, L = c.layers;
    const size_t HH = (size_t)H * H, IH = (size_t)I * H, es = esize(e->dtype);
    e->pos_emb = dmalloc(e, (size_t)c.max_positions * H * es, false);
    e->type_emb = dmalloc(e, (size_t)H * es, false);
    if (!e->pos_emb || !e->type_emb || !upload_as(e, tensors[1], (size_t)c.max_positions * H, e->pos_emb, staging) || !upload_as(e, tensors[2], H, e->type_emb, staging)) return false;
    e->eln_g = upload_f32(e, tensors[3], H); e->eln_b = upload_f32(e, tensors[4], H);
    if (!e->eln_g || !e->eln_b) return false;
    e->layers.resize(L);
    for (int l = 0; l < L; ++l) {
        const float* const* t = tensors + GLC_BERT_TENSORS_FIXED + GLC_BERT_TENSORS_PER_LAYER * l;
        LayerW& w = e->layers[l];
        if (!upload_projections(e, staging, {{&w.Wqkv, {{t[0], 3 * HH}}}, {&w.Wo, {{t[2], HH}}}, {&w.W1, {{t[6], IH}}}, {&w.W2, {{t[8], IH}}}})) return false;
        w.bqkv = upload_f32(e, t[1], 3 * (size_t)H); w.bo = upload_f32(e, t[3], H);
        w.ln1g = upload_f32(e, t[4], H); w.ln1b = upload_f32(e, t[5], H);
        w.b1 = upload_f32(e, t[7], I); w.b2 = upload_f32(e, t[9], H);
        w.ln2g = upload_f32(e, t[10], H); w.ln2b = upload_f32(e, t[11], H);
        if (!w.bqkv || !w.bo || !w.ln1g || !w.ln1b || !w.b1 || !w.b2 || !w.ln2g || !w.ln2b) return false;
    }
    return true;
}

// the value a 16-bit MFMA operand carries for f (host side of glc_launch_convert)
inline float round_as_operand(float f, int dtype) {
    if (dtype == GLC_F16) return (float)(_Float16)f;
    if (dtype == GLC_BF16) return (float)(__bf16)f;
    return f;
}

// DeBERTa-v3 backbone: upload + convert weights, the per-layer position projections and the LayerNorm folds
bool create_deberta(glc_engine* e, const float* const* tensors, float* staging) {
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter, L = c.layers, nh = c.heads, dtype = e->dtype;
    const size_t HH = (size_t)H * H, IH = (size_t)I * H;
    const int span = c.pos_buckets > 0 ? c.pos_buckets : c.max_rel_pos;
    const int P = 2 * span;
    e->P = P;
    const size_t es = esize(dtype);
    e->eln_g = upload_f32(e, tensors[1], H); e->eln_b = upload_f32(e, tensors[2], H);
    if (!e->eln_g || !e->eln_b) return false;

    // R = LayerNorm(rel_embeddings) in fp32 (HF:595-599), then to T, padded to 128 rows
    const int Ppad = round_up(P, 256);
    float* rel_f32 = upload_f32(e, tensors[3], (size_t)P * H);
    float* rg = upload_f32(e, tensors[4], H); float* rb = upload_f32(e, tensors[5], H);
    float* Rf = (float*)dmalloc(e, (size_t)Ppad * H * sizeof(float));
    void* Rt = dmalloc(e, (size_t)Ppad * H * es);
    void* vscratch = dmalloc(e, (size_t)nh * 64 * P * es);
    if (!rel_f32 || !rg || !rb || !Rf || !Rt || !vscratch) return false;
    KCHK(glc_launch_layernorm(e->stream, GLC_F32, rel_f32, Rf, rg, rb, c.ln_eps, P, H), false);
    KCHK(glc_launch_convert(e->stream, dtype, Rf, Rt, (size_t)Ppad * H), false);

    // HF:237-242: scores / sqrt(d * 3); times log2(e) so that the attention kernels can use exp2 directly
    const float inv_scale = 1.4426950408889634f / sqrtf((float)c.head_dim * 3.0f);
    std::vector<float> wq(HH), bqkv(3 * (size_t)H);
    e->layers.resize(L);
    float ln_bound = 0.f;
    for (int i = 0; i < H; ++i) ln_bound = fmaxf(ln_bound, fabsf(tensors[1][i]) * sqrtf((float)H) + fabsf(tensors[2][i]));      // the embedding LayerNorm
    for (int l = 0; l < L; ++l) {
        const float* const* t = tensors + GLC_TENSORS_FIXED + GLC_TENSORS_PER_LAYER * l;
        LayerW& w = e->layers[l];
        w.PK = dmalloc(e, (size_t)nh * P * 64 * es);
        w.PQ = dmalloc(e, (size_t)nh * P * 64 * es);
        if (!w.PK || !w.PQ) return false;
        for (size_t i = 0; i < HH; ++i) wq[i] = t[0][i] * inv_scale;   // fold log2(e)/sqrt(3d) into the query projection
        for (int i = 0; i < H; ++i) { bqkv[i] = t[1][i] * inv_scale; bqkv[H + i] = t[3][i]; bqkv[2 * H + i] = t[5][i]; }
        if (!upload_projections(e, staging, {{&w.Wqkv, {{wq.data(), HH}, {t[2], HH}, {t[4], HH}}}, {&w.Wo, {{t[6], HH}}}, {&w.W1, {{t[10], IH}}}, {&w.W2, {{t[12], IH}}}}))
            return false;
        w.bqkv = upload_f32(e, bqkv.data(), 3 * (size_t)H);
        w.bo = upload_f32(e, t[7], H); w.ln1g = upload_f32(e, t[8], H); w.ln1b = upload_f32(e, t[9], H);
        w.b1 = upload_f32(e, t[11], I); w.b2 = upload_f32(e, t[13], H);
        w.ln2g = upload_f32(e, t[14], H); w.ln2b = upload_f32(e, t[15], H);
        for (int i = 0; i < H; ++i) {       // (proactive fp8 range guard, below: the largest element a normalised row of this layer can hold)
            ln_bound = fmaxf(ln_bound, fmaxf(fabsf(t[8][i]) * sqrtf((float)H) + fabsf(t[9][i]), fabsf(t[14][i]) * sqrtf((float)H) + fabsf(t[15][i])));
        }
        if (!w.bqkv || !w.bo || !w.ln1g || !w.ln1b || !w.b1 || !w.b2 || !w.ln2g || !w.ln2b) return false;
        if (hipStreamSynchronize(e->stream) != hipSuccess) { glc_set_err("sync failed"); return false; }   // bqkv host buffer is reused
        // position projections (HF:296-302, share_att_key): PQ = query_proj(R)*log2e/sqrt(3d), PK = key_proj(R)
        GemmArgs g;
        g.A = Rt; g.W = w.Wqkv; g.bias = w.bqkv; g.Qh = w.PQ; g.Kh = w.PK; g.Vt = vscratch;
        g.Mpad = Ppad; g.N = 3 * H; g.K = H; g.Mvalid = P; g.Sp = P; g.nh = nh; g.H = H;
        g.w_presplit = e->w_presplit && dtype == GLC_F32;
        KCHK(glc_launch_gemm_auto(e->stream, dtype, EPI_QKV, g), false);
        if (e->attn_split) {      // the same tables once more as split-f16 units for the fp32 band kernel
            w.PKs = dmalloc(e, (size_t)nh * P * 64 * es);
            w.PQs = dmalloc(e, (size_t)nh * P * 64 * es);
            if (!w.PKs || !w.PQs) return false;
            g.Qh = w.PQs; g.Kh = w.PKs; g.qkv_split = 1;
            KCHK(glc_launch_gemm_auto(e->stream, dtype, EPI_QKV, g), false);
        }
        if (e->ln_fused && ((e->w_presplit && dtype == GLC_F32) || dtype != GLC_F32)) {
            // LayerNorm folded into the consumer GEMMs of the group-split pipeline (GemmArgs::a_stats):
            //   W1' = W1 diag(gamma1), c1 = W1' 1, d1 = W1 beta1 + b1            (this layer's ln1 feeds its FFN1)
            //   Wqkv' = Wqkv diag(gamma2 of layer l - 1), cq, dq likewise          (the previous layer's ln2 feeds this QKV; layer 0
            //   reads the embedding LayerNorm's output, which stays a kernel of its own)
            // (upload_projections splits the folded copies in the fp32 mode; the 16-bit modes keep plain rows of T)
            std::vector<float> wf((size_t)(I > 3 * H ? I : 3 * H) * H), cv(I > 3 * H ? I : 3 * H), dv(cv.size());
            auto fold = [&](const float* Wsrc, int rows, const float* gam, const float* bet, const float* b0, int row0) {
                for (int n = 0; n < rows; ++n) {
                    double cs = 0.0, ds = 0.0;
                    const float* wr = Wsrc + (size_t)n * H;
                    float* o = wf.data() + (size_t)(row0 + n) * H;
                    // c[n] sums the folded weights AS THE MFMA SEES THEM (rounded to T in the 16-bit modes; hi + lo in the fp32 mode is f to 2^-22):
                    // summed from the unrounded values, rstd (acc - mean c[n]) would keep a residue mean rstd sum(round(W') - W')
                    for (int k = 0; k < H; ++k) { const float f = wr[k] * gam[k]; o[k] = f; cs += (double)round_as_operand(f, dtype); ds += (double)bet[k] * (double)wr[k]; }
                    cv[row0 + n] = (float)cs; dv[row0 + n] = (float)(ds + (double)b0[row0 + n]);
                }
            };
            fold(t[10], I, t[8], t[9], t[11], 0);
            if (!upload_projections(e, staging, {{&w.W1f, {{wf.data(), IH}}}})) return false;
            w.c1 = upload_f32(e, cv.data(), I); w.d1 = upload_f32(e, dv.data(), I);
            if (!w.c1 || !w.d1) return false;
            if (l > 0) {
                const float* const* tp = tensors + GLC_TENSORS_FIXED + GLC_TENSORS_PER_LAYER * (l - 1);
                fold(wq.data(), H, tp[14], tp[15], bqkv.data(), 0);       // wq / bqkv still hold this layer's scaled query projection
                fold(t[2], H, tp[14], tp[15], bqkv.data(), H);
                fold(t[4], H, tp[14], tp[15], bqkv.data(), 2 * H);
                if (!upload_projections(e, staging, {{&w.Wqkvf, {{wf.data(), 3 * HH}}}})) return false;
                w.cq = upload_f32(e, cv.data(), 3 * (size_t)H); w.dq = upload_f32(e, dv.data(), 3 * (size_t)H);
                if (!w.cq || !w.dq) return false;
            }
            if (hipStreamSynchronize(e->stream) != hipSuccess) { glc_set_err("sync failed"); return false; }   // host vectors are reused
        }
        if (e->mx_built && w.PKs && w.PQs) {
            // MX pipeline: the GX copies of the projection weights are built by the first forward that takes the pipeline (build_mx_weights);
            // the position tables are converted here (small, and the range guard decides per layer at load): PQ travels as (hi8 | lo8), PK as (lo8 | hi8)
            // (each buffer = the tile images twice: [MX steps as 32 bytes per lane — the Q / K tile format | planar: MX steps as two 16-byte planes,
            //  every piece of a row at the SAME per-lane offset, glc_layout.h] — the band loop's requests read the second copy, round 6)
            w.PKm = dmalloc(e, 2 * (size_t)nh * P * 64 * es);
            w.PQm = dmalloc(e, 2 * (size_t)nh * P * 64 * es);
            // (fp8 range guard at load: a table value beyond the e4m3 range keeps this layer's attention on split units)
            unsigned seen = 0;
            const char* pm = !init_range_guard(e) ? "range guard: allocation failed" : (w.PKm && w.PQm) ? glc_launch_units_to_mxt(e->stream, w.PKs, w.PKm, nh * (P / 32), 0, e->d_gxsat) : "MX position tables: allocation failed";
            if (!pm) pm = glc_launch_units_to_mxt(e->stream, w.PQs, w.PQm, nh * (P / 32), 1, e->d_gxsat);
            if (!pm) pm = glc_launch_units_to_mxt(e->stream, w.PKs, (unsigned char*)w.PKm + (size_t)nh * P * 64 * es, nh * (P / 32), 0, nullptr, 1);
            if (!pm) pm = glc_launch_units_to_mxt(e->stream, w.PQs, (unsigned char*)w.PQm + (size_t)nh * P * 64 * es, nh * (P / 32), 1, nullptr, 1);
            if (!pm && (hipMemcpyAsync(&seen, e->d_gxsat, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess)) pm = "MX position tables: readback failed";
            KCHK(pm, false);
            if (seen != e->gxsat_seen[0]) { e->gxsat_seen[0] = seen; dfree(e, w.PKm); dfree(e, w.PQm); w.PKm = w.PQm = nullptr; }
        }
    }
    // Proactive fp8 range guard: the activation rows of the MX pipeline are LayerNorm outputs (and raw sums built from
    // them); an element of a normalised row is at most |gamma| sqrt(H) + |beta|.  A checkpoint whose gains put that bound beyond e4m3's
    // 448 (outlier channels) starts with the activation exponent the reactive guard would reach after one repeated forward — no request
    // pays the 2-3x repeat.  (The bound is the worst case of one spiked row; the reactive guard stays in place behind it.)
    if (e->mx_built && ln_bound > 448.0f && e->act_sc == 0) {
        e->act_sc = kActScLow;
        fprintf(stderr, "gliclass: LayerNorm gains of this checkpoint allow activations up to %.0f (beyond the fp8 range of the MX operand images, 448); "
                        "this engine's activation rows carry exponent %d (|x| up to %d) from the start\n", ln_bound, kActScLow, 448 << -kActScLow);
    }
    if (hipStreamSynchronize(e->stream) != hipSuccess) { glc_set_err("sync failed"); return false; }   // (the position projections read the load-time tables)
    dfree(e, rel_f32); dfree(e, rg); dfree(e, rb); dfree(e, Rf); dfree(e, Rt); dfree(e, vscratch);
    return true;
}

bool check_shape(const glc_engine* e, int B, int S, int C) {
    if (B <= 0 || S <= 0 || C < 0) { glc_set_err("forward: B and S must be positive, C non-negative"); return false; }
    if ((long long)B * round_up(S, 64) > (1ll << 30)) { glc_set_err("forward: batch too large"); return false; }
    // BERT backbone: the position table has max_positions rows and the ids start at pos_offset (never a clamp)
    if (e->cfg.backbone == GLC_BACKBONE_BERT && S > e->cfg.max_positions - e->cfg.pos_offset) {
        glc_set_err("forward: S = " + std::to_string(S) + " tokens per row, but the position table of this BERT backbone holds max_positions - pos_offset = " +
                    std::to_string(e->cfg.max_positions - e->cfg.pos_offset));
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

const char* glc_last_error(void) { return g_err.c_str(); }

int glc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* modeling_deberta_v2.py:57-69 (make_log_bucket_position) + :318 clamp; float32 arithmetic like torch */
void glc_delta_table(int S, int bucket_size, int max_position, int32_t* out) {
    const int span = bucket_size > 0 ? bucket_size : max_position;
    const int mid = bucket_size / 2;
    const float den = (bucket_size > 0 && max_position > 0) ? logf((float)(((double)max_position - 1.0) / (double)mid)) : 1.f;
    for (int r = -(S - 1); r <= S - 1; ++r) {
        int bk = r;
        if (bucket_size > 0 && max_position > 0) {
            const int ar = r < 0 ? -r : r;
            if (ar > mid) {
                const float lp = ceilf(logf((float)ar / (float)mid) / den * (float)(mid - 1)) + (float)mid;
                bk = (int)(r < 0 ? -lp : lp);
            }
        }
        int v = bk + span;
        out[r + S - 1] = v < 0 ? 0 : (v > 2 * span - 1 ? 2 * span - 1 : v);
    }
}

/* modeling_t5.py T5Attention._relative_position_bucket (T5:217-262) with bidirectional=True, relative_position = key - query; float32
 * arithmetic like torch: log(rp / max_exact) / log(max_distance / max_exact) * (half - max_exact), truncated (.to(torch.long)) */
void glc_t5_bucket_table(int S, int num_buckets, int max_distance, int32_t* out) {
    const int half = num_buckets / 2, max_exact = half / 2;
    const float den = (float)log((double)max_distance / (double)max_exact);      // (math.log of two Python numbers, then a float32 operand)
    for (int r = -(S - 1); r <= S - 1; ++r) {
        const int ar = r < 0 ? -r : r;
        int bk = r > 0 ? half : 0;
        if (ar < max_exact) bk += ar;
        else {
            const float lg = logf((float)ar / (float)max_exact) / den * (float)(half - max_exact);
            const int big = max_exact + (int)lg;
            bk += big < half - 1 ? big : half - 1;
        }
        out[r + S - 1] = bk;
    }
}

glc_engine* glc_engine_create(const glc_model_config* cfg, const float* const* tensors, int n_tensors, int device, int dtype) {
    if (!cfg || !tensors) { glc_set_err("engine_create: null argument"); return nullptr; }
    if (dtype != GLC_F32 && dtype != GLC_BF16 && dtype != GLC_F16) { glc_set_err("engine_create: bad dtype"); return nullptr; }
    if ((cfg->qk_norm & ~1) || (cfg->attn_bias & ~1)) { glc_set_err("engine_create: qk_norm and attn_bias must be 0 or 1"); return nullptr; }
    if (cfg->qk_norm && cfg->backbone != GLC_BACKBONE_DECODER) { glc_set_err("engine_create: qk_norm = 1 (per-head RMSNorm on Q and K) exists on the decoder backbone only"); return nullptr; }
    const bool seqcls = cfg->head_kind == GLC_HEAD_SEQCLS;
    if (cfg->head_kind != GLC_HEAD_GLICLASS && !seqcls) { glc_set_err("engine_create: head_kind must be 0 (GLiClass head) or 1 (sequence classification)"); return nullptr; }
    if (!seqcls && (cfg->cls_labels || cfg->cls_act || cfg->cls_norm || cfg->cls_dense)) {
        glc_set_err("engine_create: cls_labels, cls_act, cls_norm and cls_dense belong to head_kind = 1 (sequence classification); head_kind = 0 needs them 0"); return nullptr;
    }
    if (seqcls) {
        // (before anything touches a device: a refusal of the configuration alone)
        if (cfg->backbone == GLC_BACKBONE_DECODER) { glc_set_err("engine_create: head_kind = 1 (sequence classification) is not available on the decoder backbone (decoder ...ForSequenceClassification heads are out of scope)"); return nullptr; }
        if (cfg->backbone == GLC_BACKBONE_T5) { glc_set_err("engine_create: head_kind = 1 (sequence classification) is not available on the T5 backbone (T5ForSequenceClassification needs the decoder stack)"); return nullptr; }
        if (cfg->cls_labels < 1 || cfg->cls_labels > GLC_CLS_MAX_LABELS) { glc_set_err("engine_create: cls_labels must be 1 .. 1024"); return nullptr; }
        if (cfg->cls_act < GLC_CLS_ACT_NONE || cfg->cls_act > GLC_CLS_ACT_GELU) { glc_set_err("engine_create: cls_act must be 0 (none), 1 (tanh) or 2 (gelu)"); return nullptr; }
        if ((cfg->cls_norm & ~1) || (cfg->cls_dense & ~1)) { glc_set_err("engine_create: cls_norm and cls_dense must be 0 or 1"); return nullptr; }
        if (cfg->pooling != GLC_POOL_FIRST && cfg->pooling != GLC_POOL_AVG) { glc_set_err("engine_create: head_kind = 1 pools 'first' or 'avg' (pooling)"); return nullptr; }
        if (cfg->hidden > 2048) { glc_set_err("engine_create: head_kind = 1 needs hidden <= 2048"); return nullptr; }
    }
    if (n_tensors != glc_num_tensors_cfg(cfg)) { glc_set_err("engine_create: wrong tensor count"); return nullptr; }
    {
        // the optional slots of the sequence-classification head may be null (include/gliclass_hip.h); nothing else may
        const int h0 = n_tensors - GLC_TENSORS_CLS_HEAD;
        for (int i = 0; i < n_tensors; ++i) {
            const int k = seqcls ? i - h0 : -1;
            const bool must_null = (k == 0 || k == 1) ? !cfg->cls_dense : (k == 2 || k == 3) ? !cfg->cls_norm : false;
            const bool may_null = must_null || k == 1 || k == 3 || k == 5;
            if (must_null && tensors[i]) { glc_set_err("engine_create: a dense / norm tensor of the sequence-classification head is given although cls_dense / cls_norm = 0"); return nullptr; }
            if (!tensors[i] && !may_null) { glc_set_err("engine_create: null tensor"); return nullptr; }
        }
    }
    const bool dec = cfg->backbone == GLC_BACKBONE_DECODER, mb = cfg->backbone == GLC_BACKBONE_MODERNBERT, bert = cfg->backbone == GLC_BACKBONE_BERT;
    const bool t5 = cfg->backbone == GLC_BACKBONE_T5;
    if (cfg->backbone != GLC_BACKBONE_DEBERTA && !dec && !mb && !bert && !t5) { glc_set_err("engine_create: unknown backbone"); return nullptr; }
    if (t5 && (cfg->head_dim != 64 || cfg->heads < 1 || cfg->layers < 1 || cfg->rel_buckets < 4 || cfg->rel_buckets % 4 || cfg->rel_buckets > (1 << 16) ||
               cfg->rel_max_distance <= cfg->rel_buckets / 4 || cfg->pad_id < 0 || cfg->pad_id >= cfg->vocab)) {
        glc_set_err("engine_create: T5 backbone needs head_dim 64, rel_buckets a multiple of 4 and rel_max_distance > rel_buckets / 4"); return nullptr;
    }
    if (bert && (cfg->head_dim != 64 || cfg->hidden != cfg->heads * 64 || cfg->layers < 1 || cfg->type_vocab < 1 || cfg->pos_offset < 0 || cfg->pad_id < 0 ||
                 cfg->pad_id >= cfg->vocab || (cfg->pos_offset != 0 && cfg->pos_offset != cfg->pad_id + 1) || cfg->max_positions - cfg->pos_offset < 1)) {
        glc_set_err("engine_create: BERT backbone needs head_dim 64, type_vocab >= 1, pos_offset 0 or pad_id + 1 and max_positions > pos_offset"); return nullptr;
    }
    if (mb && (cfg->head_dim != 64 || cfg->hidden != cfg->heads * 64 || cfg->local_window < 0 || (cfg->local_window > 0 && cfg->global_every < 1) ||
               cfg->rope_theta <= 1.f || (cfg->local_window > 0 && cfg->rope_theta_local <= 1.f))) {
        glc_set_err("engine_create: ModernBERT backbone needs head_dim 64, local_window >= 0, global_every >= 1 and RoPE bases > 1"); return nullptr;
    }
    if (!dec && !mb && !bert && !t5 && (cfg->head_dim != 64 || cfg->hidden != cfg->heads * 64)) { glc_set_err("engine_create: head_dim must be 64 (all DeBERTa-v3 backbones)"); return nullptr; }
    if (dec && ((cfg->head_dim != 64 && cfg->head_dim != 128) || cfg->heads <= 0 || cfg->kv_heads < 0 ||
                cfg->heads % (cfg->kv_heads > 0 ? cfg->kv_heads : cfg->heads) || cfg->rope_theta <= 1.f)) {
        glc_set_err("engine_create: decoder backbone needs head_dim 64 or 128, heads % kv_heads == 0 and rope_theta > 1"); return nullptr;
    }
    // (ModernBERT: the GeGLU width may be a multiple of 64 — modernbert-large's 2624 — the fused [input | gate] projection is 2I wide)
    if (cfg->hidden % 128 || cfg->inter % (mb ? 64 : 128)) { glc_set_err("engine_create: hidden and intermediate sizes must be multiples of 128 (ModernBERT: 64)"); return nullptr; }
    if (cfg->pooling < GLC_POOL_FIRST || cfg->pooling > GLC_POOL_LAST || cfg->scorer < GLC_SCORER_DOT || cfg->scorer > GLC_SCORER_MLP) {
        glc_set_err("engine_create: pooling must be 'first', 'avg' or 'last' and the scorer 'simple', 'weighted-dot' or 'mlp'"); return nullptr;
    }
    int ndev = glc_device_count();
    if (ndev <= 0) { glc_set_err("engine_create: no HIP device visible (this engine has no CPU path)"); return nullptr; }
    if (device < 0 || device >= ndev) { glc_set_err("engine_create: bad device ordinal"); return nullptr; }
    HIPCHK(hipSetDevice(device), nullptr);
    if (dec) {
        const size_t NQ = (size_t)cfg->heads * cfg->head_dim, NKV = (size_t)(cfg->kv_heads > 0 ? cfg->kv_heads : cfg->heads) * cfg->head_dim;
        if (NQ % 128 || NKV % 64 || (NQ + 2 * NKV) % 128) { glc_set_err("engine_create: decoder projection widths must be multiples of 128"); return nullptr; }
    }

    glc_engine* e = new glc_engine();
    e->cfg = *cfg; e->dtype = dtype; e->device = device;
    if (e->cfg.kv_heads <= 0) e->cfg.kv_heads = e->cfg.heads;
    if (t5) e->t5_heads = (cfg->heads + 1) / 2 * 2;
    if (const char* pv = getenv("GLICLASS_PRUNE_LAST")) e->prune_last = atoi(pv) != 0;
    { const char* gv = getenv("GLICLASS_F32_GEMM"); e->w_presplit = !(gv && !strcmp(gv, "native")) ; }   // hidden and inter are multiples of 128 (checked above)
    { const char* av = getenv("GLICLASS_F32_ATTN"); e->dec_split = dtype == GLC_F32 && (dec || mb || bert || t5) && !(av && !strcmp(av, "native")); }
    { const char* av = getenv("GLICLASS_F32_ATTN"); e->attn_split = dtype == GLC_F32 && cfg->backbone == GLC_BACKBONE_DEBERTA && !(av && !strcmp(av, "native")); }
    if (const char* lv = glc_dev_env("GLC_LNF")) e->ln_fused = atoi(lv) != 0;      // developer A/B switch
    // MX cross-term pipeline (docs/LOG_r01-r05.md §3e) — the default arithmetic of the large forwards of the default mode since round 3: the
    // projections of the full layers run a_hi*w_hi in f16 MFMAs and both cross terms in one block-scaled fp8 MFMA (per-label
    // probabilities within 1e-4 of the split-f16 arithmetic, measured; the bar is 1e-3).  GLICLASS_MX=0: split-f16 projections
    // everywhere (three f16 MFMAs per product, ~1e-5); GLICLASS_MX=build: GX weight copies built, pipeline off until glc_debug_set_mx.
    {
        const char* mv = getenv("GLICLASS_MX");
        e->mx_env = !mv ? 0 : !strcmp(mv, "0") ? 1 : !strcmp(mv, "build") ? 2 : 0;
        const bool eligible = dec ? (dtype == GLC_F32 && e->w_presplit && e->dec_split && e->ln_fused && cfg->hidden % 256 == 0 && (2 * cfg->inter) % 256 == 0 && cfg->inter % 32 == 0)
                                  : (dtype == GLC_F32 && e->w_presplit && e->attn_split && e->ln_fused && cfg->hidden % 256 == 0 && cfg->inter % 256 == 0 && cfg->layers >= 2);
        e->mx_built = eligible && !mb && !bert && !t5 && !(mv && !strcmp(mv, "0"));      // (ModernBERT: opt-in, glc_engine_enable_mx; BERT, T5: no MX pipeline)
        e->mx = e->mx_built && !(mv && !strcmp(mv, "build"));
        if (const char* av = glc_dev_env("GLC_MX_ATTN")) e->mx_attn = atoi(av) != 0;      // developer A/B switch
        if (const char* av = glc_dev_env("GLC_DEC_ROPE_EPI")) e->dec_rope_epi = atoi(av) != 0;      // developer A/B switch
    }
    if (const char* gv = glc_dev_env("GLC_GS")) { const int g = atoi(gv); e->gs_mode = g < 0 ? 0 : (g > 2 ? 2 : g); }       // developer A/B switch
    if (const char* bv = getenv("GLICLASS_LENGTH_BUCKETS")) { const int g = atoi(bv); e->max_buckets = g < 1 ? 1 : (g > 64 ? 64 : g); }
    // decoder SwiGLU / ModernBERT GeGLU in the epilogue of the staggered 256-tile GEMM when the shapes allow it (16-bit operands; fp32 mode: the
    // group-split 256-tile GEMM has the same epilogue, its small-forward fallback un-fuses on the interleaved columns)
    const int H = cfg->hidden, I = cfg->inter;
    e->fused_swiglu = (dec || mb) && (dtype != GLC_F32 || (e->w_presplit && e->dec_split && H % 256 == 0)) && (2 * I) % 256 == 0 && H % 32 == 0 &&
                      I % 16 == 0 && glc_dev_env("GLC_NO_FUSED_SWIGLU") == nullptr;

    float* staging = nullptr;      // host f32 -> device T goes through it (upload_as)
    struct StagingGuard { float*& p; ~StagingGuard() { (void)hipFree(p); } } staging_guard{staging};      // (every exit path)
    auto fail = [e]() -> glc_engine* { glc_engine_destroy(e); return nullptr; };
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { glc_set_err("stream create failed"); return fail(); }
    if (hipEventCreate(&e->t0) != hipSuccess || hipEventCreate(&e->t1) != hipSuccess) { glc_set_err("event create failed"); return fail(); }
    if (hipMalloc((void**)&staging, staging_floats(e->cfg) * sizeof(float)) != hipSuccess) { glc_set_err("staging alloc failed"); return fail(); }
    const size_t nemb = (size_t)cfg->vocab * H;           // the token embeddings (HF:518-562)
    e->emb = dmalloc(e, nemb * esize(dtype), false);
    if (!e->emb || !upload_as(e, tensors[0], nemb, e->emb, staging)) return fail();
    const bool loaded = dec ? create_decoder(e, tensors, staging) : mb ? create_modernbert(e, tensors, staging) : bert ? create_bert(e, tensors, staging)
                            : t5 ? create_t5(e, tensors, staging) : create_deberta(e, tensors, staging);
    if (!loaded || !(seqcls ? upload_cls_head(e, tensors + n_tensors - GLC_TENSORS_CLS_HEAD)
                            : upload_head(e, tensors + n_tensors - GLC_TENSORS_HEAD - glc_num_scorer_tensors(cfg->scorer)))) return fail();
    // ModernBERT: the MX pipeline is opt-in; the environment makes the call glc_engine_enable_mx documents (read once, here).  An engine it does
    // not fit stays as it is: not an error.
    if (mb) {
        const char* ov = getenv("GLICLASS_MX_MODERNBERT");
        if (ov && !strcmp(ov, "1") && glc_engine_enable_mx(e) != 0)
            fprintf(stderr, "gliclass: GLICLASS_MX_MODERNBERT=1 has no effect on this engine (%s)\n", glc_last_error());
    }
    // Captured-graph replay is opt-in as well; the environment makes the call glc_engine_set_graph_replay documents (read once, here)
    if (const char* gv = getenv("GLICLASS_GRAPH_REPLAY"))
        if (!strcmp(gv, "1") && glc_engine_set_graph_replay(e, 1) != 0)
            fprintf(stderr, "gliclass: GLICLASS_GRAPH_REPLAY=1 has no effect on this engine (%s)\n", glc_last_error());
    // ... and so is the MX pipeline for forwards below the 256 tile's fill rule (glc_engine_set_mx_small_forwards)
    if (const char* sv = getenv("GLICLASS_MX_SMALL"))
        if ((!strcmp(sv, "1") || !strcmp(sv, "2")) && glc_engine_set_mx_small_forwards(e, atoi(sv)) != 0)
            fprintf(stderr, "gliclass: GLICLASS_MX_SMALL=%s has no effect on this engine (%s)\n", sv, glc_last_error());
    return e;
}

/* Opt-in MX pipeline of the ModernBERT backbone (include/gliclass_hip.h). */
int glc_engine_enable_mx(glc_engine* e) {
    if (!e) { glc_set_err("enable_mx: null engine"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->cfg.backbone == GLC_BACKBONE_BERT) { glc_set_err("enable_mx: the BERT backbone has no MX pipeline (its forwards run the split-f16 / 16-bit kernels)"); return -1; }
    if (e->cfg.backbone == GLC_BACKBONE_T5) { glc_set_err("enable_mx: the T5 backbone has no MX pipeline (its forwards run the split-f16 / 16-bit kernels)"); return -1; }
    if (e->cfg.backbone != GLC_BACKBONE_MODERNBERT) {
        if (e->mx_built) return 0;
        glc_set_err("enable_mx: the MX pipeline is not available to this engine (shapes, dtype, or GLICLASS_MX=0 at creation)"); return -1;
    }
    if (e->mx_built && e->mx_ready) return 0;
    graph_clear(e);
    const glc_model_config& c = e->cfg;
    const int H = c.hidden, I = c.inter;
    const char* why = nullptr;
    if (e->dtype != GLC_F32) why = "the MX pipeline runs in the fp32 mode only (this engine's dtype is 16-bit)";
    else if (e->mx_env == 1) why = "GLICLASS_MX=0 was set when the engine was created";
    else if (!e->w_presplit || !e->dec_split) why = "it needs the split-f16 weights and attention (GLICLASS_F32_GEMM / GLICLASS_F32_ATTN = native were set at creation)";
    else if (c.head_dim != 64) why = "head_dim must be 64";
    else if (H % 256) why = "the hidden size must be a multiple of 256";
    else if ((2 * I) % 256 || I % 32) why = "twice the GeGLU width must be a multiple of 256 (modernbert-large: 2 x 2624 = 5248 is not) and the width a multiple of 32";
    else if (!e->fused_swiglu) why = "the GeGLU epilogue is switched off for this engine";
    else if (e->keep_hidden) why = "keep_hidden is on (the hidden-state dump needs plain rows)";
    if (why) { glc_set_err(std::string("enable_mx: ") + why); return -1; }
    HIPCHK(hipSetDevice(e->device), -1);
    if (!init_range_guard(e)) return -1;
    if (!e->splitk_ws) {                                    // (the scratch word of the weight conversion: ensure_capacity's workspace)
        e->splitk_ws_bytes = (size_t)64 << 20;
        e->splitk_ws = (float*)dmalloc(e, e->splitk_ws_bytes, false);
        if (!e->splitk_ws) { e->splitk_ws_bytes = 0; return -1; }
    }
    e->mx_built = true;
    if (!build_mx_weights(e)) { glc_set_err(std::string("enable_mx: the GX weight copies could not be built (") + glc_last_error() + ")"); return -1; }      // (mx_built is off again)
    e->mx = e->mx_env != 2;                                 // GLICLASS_MX=build: copies built, pipeline off until glc_debug_set_mx
    // Proactive activation exponent (as create_deberta): an element of a normalised row is at most |gamma| sqrt(H)
    if (e->mb_ln_bound > 448.0f && e->act_sc == 0) {
        e->act_sc = kActScLow;
        fprintf(stderr, "gliclass: LayerNorm gains of this checkpoint allow activations up to %.0f (beyond the fp8 range of the MX operand images, 448); "
                        "this engine's activation rows carry exponent %d (|x| up to %d) from the start\n", e->mb_ln_bound, kActScLow, 448 << -kActScLow);
    }
    return 0;
}

void glc_engine_destroy(glc_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    graph_clear(e);
    for (void* p : e->allocs) (void)hipFree(p);
    if (e->h_gxsat) (void)hipHostFree(e->h_gxsat);
    for (auto& v : e->evs) { (void)hipEventDestroy(v.a); (void)hipEventDestroy(v.b); }
    if (e->t0) (void)hipEventDestroy(e->t0);
    if (e->t1) (void)hipEventDestroy(e->t1);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

// One padded batch: H2D, launch sequence, D2H of logits [B, c_alloc] and per-row class-token counts.  Caller holds e->mu.
// The stream's work is complete and a device-resident forward's counter copy sits in the pinned slot: compare, remember the verdict for
// glc_engine_sync / glc_engine_device_forward_valid, and give the guard's answer (rows only: exponent kActScLow; tiles, or rows again: split-f16).
static void settle_device_range_check(glc_engine* e) {
    e->fp8_device_pending = false;
    const bool rows = e->h_gxsat[0] != e->gxsat_seen[0], tiles = e->h_gxsat[1] != e->gxsat_seen[1];
    e->gxsat_seen[0] = e->h_gxsat[0]; e->gxsat_seen[1] = e->h_gxsat[1];
    if (!rows && !tiles) return;
    graph_clear(e);      // (the guard's answer changes the arithmetic of every later forward)
    if (rows && !tiles && e->act_sc == 0) { e->act_sc = kActScLow; e->device_invalid = 1; }
    else { e->fp8_sticky_off = true; e->device_invalid = 2; }
}

static int forward_one(glc_engine* e, const int64_t* ids, const int64_t* mask, int B, int S, float* logits, int c_alloc, int* cnt) {
    if (!ensure_capacity(e, B, S, c_alloc)) return -1;
    const size_t nb = (size_t)B * S * sizeof(int64_t);
    HIPCHK(hipMemcpyAsync(e->d_ids, ids, nb, hipMemcpyHostToDevice, e->stream), -1);
    HIPCHK(hipMemcpyAsync(e->d_mask, mask, nb, hipMemcpyHostToDevice, e->stream), -1);
    // Every matrix product runs on f16 / bf16 MFMA operands (the fp32 mode as split-f16 pairs), so an activation beyond the operand
    // range (|x| > 65504 for f16) turns into inf / NaN silently.  A result the reference's fp32 graph would not produce must not be
    // returned as if it were one.  With the norm folded into the GEMMs (docs/LOG_r01-r05.md §3d) the RAW residual stream is such an operand — a
    // pre-norm decoder's massive-activation channels can leave the f16 range although every normalised row is tiny — so a non-finite
    // result of a folded forward is retried ONCE with the norms as kernels of their own (residual stream plain fp32, only normalised
    // rows split); what is still non-finite then fails the call.  (fp32 mode: GLICLASS_F32_GEMM=native GLICLASS_F32_ATTN=native run the fp32 MFMAs.)
    // fp8 range (round 4): the MX pipeline's operand images carry e4m3 parts with exponent 0; an activation beyond 448 has no image there (NaN
    // from 464 on: the producers do not clamp, glc_common.h gx_split8).  Every producer counts such elements (glc_common.h gx_range_note);
    // a forward that counted any is repeated ONCE on the split-f16 kernels (operands up to 65504, the LayerNorm fold kept).  After kFp8Sticky
    // consecutive forwards that needed it the engine leaves the MX pipeline for good: the model has outlier channels, paying twice per forward is pointless.
    struct Restore {      // every exit path puts the engine's switches back (a HIP error inside a retry must not leave it unfused / off MX)
        glc_engine* e; bool fused, mx;
        ~Restore() { e->ln_fused = fused; e->mx = mx; }
    } restore{e, e->ln_fused, e->mx};
    // (a device-resident forward that has not been through glc_engine_sync yet: settle its range check first — this forward's own
    //  counter readings would otherwise make the pinned copy look stale and glc_engine_sync report a range error that never happened;
    //  and BEFORE the sticky switch is read: a verdict that turns it on must already keep this forward off the MX pipeline)
    if (e->fp8_device_pending) {
        HIPCHK(hipStreamSynchronize(e->stream), -1);
        settle_device_range_check(e);
    }
    if (e->fp8_sticky_off) e->mx = false;
    unsigned sat_now[2] = {e->gxsat_seen[0], e->gxsat_seen[1]};
    bool tried_unfused = false, tried_split = false, tried_low = false;
    for (int attempt = 0; attempt < 4; ++attempt) {      // at most: MX, MX with exponent kActScLow, split-f16, norms unfused
        if (!graph_forward(e, e->d_ids, e->d_mask, B, S, c_alloc, e->d_logits)) return -1;
        HIPCHK(hipMemcpyAsync(cnt, e->cls_cnt, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, e->stream), -1);
        if (c_alloc > 0) HIPCHK(hipMemcpyAsync(logits, e->d_logits, (size_t)B * c_alloc * sizeof(float), hipMemcpyDeviceToHost, e->stream), -1);
        HIPCHK(hipMemcpyAsync(sat_now, e->d_gxsat, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, e->stream), -1);
        HIPCHK(hipStreamSynchronize(e->stream), -1);
        bool finite = true;
        for (size_t i = 0, n = (size_t)B * (c_alloc > 0 ? c_alloc : 0); i < n && finite; ++i) finite = isfinite(logits[i]);
        // the two words of the guard: activation rows (their exponent can be lowered) and Q / K / V tiles (exponent 0: only the split kernels help)
        const bool sat_rows = sat_now[0] != e->gxsat_seen[0], sat_tiles = sat_now[1] != e->gxsat_seen[1];
        const bool sat = sat_rows || sat_tiles;
        e->gxsat_seen[0] = sat_now[0]; e->gxsat_seen[1] = sat_now[1];
        if (sat_rows && !sat_tiles && e->last_mx && e->act_sc == 0 && !tried_low) {      // first answer: activation rows with exponent kActScLow, still on the MX pipeline (kept for this engine)
            tried_low = true;
            graph_clear(e);
            e->act_sc = kActScLow;
            e->fp8_retries++;
            fprintf(stderr, "gliclass: activations beyond the fp8 range of the MX operand images (|x| > 448); this engine's activation rows now carry exponent %d (|x| up to %d)\n", kActScLow, 448 << -kActScLow);
            continue;
        }
        if (sat && e->last_mx && !tried_split) {      // (before the non-finite check: beyond 464 the unclamped e4m3 parts are NaN — glc_common.h gx_split8 — so such a forward may well be non-finite)
            tried_split = true;
            graph_clear(e);
            e->mx = false;                  // retry: three f16 MFMAs per product, operands up to 65504
            e->fp8_retries++;
            if (++e->fp8_streak >= kFp8Sticky && !e->fp8_sticky_off) {
                e->fp8_sticky_off = true;
                fprintf(stderr, "gliclass: activations beyond the fp8 range of the MX operand images (|x| > 448) in %d consecutive forwards; this engine now runs the split-f16 arithmetic (as GLICLASS_MX=0)\n", e->fp8_streak);
            }
            continue;
        }
        if (!finite && !tried_unfused && e->dtype == GLC_F32 && e->last_lnf) {
            tried_unfused = true;
            graph_clear(e);
            e->ln_fused = false;            // retry: norms unfused (this also leaves the MX pipeline)
            e->range_retries++;
            continue;
        }
        if (e->last_mx && !sat) e->fp8_streak = 0;
        break;
    }
    if (e->profile) prof_collect(e);        // (the attempt whose result is returned)
    for (size_t i = 0, n = (size_t)B * (c_alloc > 0 ? c_alloc : 0); i < n; ++i)
        if (!isfinite(logits[i])) {
            glc_set_err("forward: non-finite logit (row " + std::to_string(i / c_alloc) + "): an activation left the range of the " +
                    (e->dtype == GLC_BF16 ? "bf16" : "f16") + " MFMA operands" +
                    (e->dtype == GLC_F32 ? "; set GLICLASS_F32_GEMM=native GLICLASS_F32_ATTN=native for the fp32-MFMA kernels" : "; use GLICLASS_DTYPE=f32 or bf16"));
            return -1;
        }
    return 0;
}

// Length bucketing: the reference pads every row of a batch to the longest one
// (/root/reference/src/tokenizer.c:44-54).  Rows are independent end to end and columns past a row's last attended token
// contribute nothing, so a ragged batch can run as a few groups of similar length, each padded only to ITS longest row.
// Plans the partition of the rows (sorted by length) into <= max_groups contiguous groups that minimises
// sum_g ( BucketCost(n_g * roundup(len_g, 64)) + kBucketOverheadRows ); returns the group boundaries in `cuts`
// (indices into `order`).  A coarse cost model in units of padded token rows: the 256-row GEMM tiles of the narrowest
// projection (N = hidden) fill the chip in whole waves of `quantum` = 256 * CUs / (hidden / 256) rows — measured: config c3's
// 65 536 rows are exactly three waves, and two forwards of 32 768 rows each take LONGER than one of 65 536 — and every
// extra forward costs about 1 k rows of fixed work (head, pruned last layer, launch sequence).
constexpr int kBucketOverheadRows = 1024;
// cost of a forward of `rows` padded token rows, in row units: its 256-row tiles of the N = hidden projections run in whole
// waves over the CUs (256 CUs assumed when no device is visible)
struct BucketCost {
    int ncu = 256, nt = 1;
    explicit BucketCost(int hidden) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ncu = n;
        nt = hidden / 256 > 0 ? hidden / 256 : 1;
    }
    long long operator()(long long rows) const {
        const long long blocks = (rows + 255) / 256 * nt, waves = (blocks + ncu - 1) / ncu;
        return waves * 256 * ncu / nt;
    }
};

static void plan_buckets(const std::vector<int>& len, int max_groups, const BucketCost& cost, std::vector<int>& order, std::vector<int>& cuts) {
    const int B = (int)len.size();
    order.resize(B);
    for (int i = 0; i < B; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len[a] > len[b]; });     // longest first
    auto sp = [&](int i) { return round_up(len[order[i]] > 0 ? len[order[i]] : 1, 64); };
    const int G = max_groups < 1 ? 1 : (max_groups > B ? B : max_groups);
    // best[g][i]: minimal cost of covering rows [i, B) with exactly g groups; a group [i, j) costs (j - i) * sp(i)
    const long long INF = 1ll << 60;
    std::vector<std::vector<long long>> best(G + 1, std::vector<long long>(B + 1, INF));
    std::vector<std::vector<int>> nxt(G + 1, std::vector<int>(B + 1, B));
    for (int g = 0; g <= G; ++g) best[g][B] = g == 0 ? 0 : INF;
    for (int g = 1; g <= G; ++g)
        for (int i = B - 1; i >= 0; --i)
            for (int j = i + 1; j <= B; ++j) {
                if (best[g - 1][j] >= INF) continue;
                const long long rows = (long long)(j - i) * sp(i);
                const long long c = cost(rows) + kBucketOverheadRows + best[g - 1][j];
                if (c < best[g][i]) { best[g][i] = c; nxt[g][i] = j; }
            }
    int gbest = 1;
    for (int g = 2; g <= G; ++g) if (best[g][0] < best[gbest][0]) gbest = g;
    cuts.clear();
    for (int g = gbest, i = 0; g >= 1 && i < B; --g) { cuts.push_back(i); i = nxt[g][i]; }
    cuts.push_back(B);
}

int glc_engine_forward(glc_engine* e, const int64_t* ids, const int64_t* mask, int B, int S, float* logits, int c_alloc, int* c_out) {
    if (!e || !ids || !mask || (!logits && c_alloc > 0)) { glc_set_err("forward: null argument"); return -1; }
    if (!check_shape(e, B, S, c_alloc)) return -1;
    const bool seqcls = e->cfg.head_kind == GLC_HEAD_SEQCLS;
    const int K = e->cfg.cls_labels;
    if (seqcls && c_alloc < K) {
        glc_set_err("forward: this engine has a sequence-classification head with " + std::to_string(K) + " labels: c_alloc = " + std::to_string(c_alloc) + " is too small (c_alloc >= cls_labels)");
        return -1;
    }
    // the head writes rows of K logits: the forward runs on the caller's buffer as [B, K], and a wider stride is made at the end, in place
    // and from the last row down (columns k >= K of a row are then unspecified)
    const int c_caller = c_alloc;
    if (seqcls) c_alloc = K;
    auto finish = [&]() {
        if (c_out) *c_out = K;
        for (int b = B - 1; b >= 1 && c_caller > K; --b) memmove(logits + (size_t)b * c_caller, logits + (size_t)b * K, (size_t)K * sizeof(float));
    };
    // A class token under attention_mask 0 is outside the contract: its hidden state would be a padding-QUERY row (HF: uniform
    // attention over every position), which this engine does not compute — refuse instead of returning a different number.  The
    // reference's tokenizer never produces it (mask 1 on every real token, /root/reference/src/tokenizer.c:77-79).
    for (size_t i = 0, n = seqcls ? 0 : (size_t)B * S; i < n; ++i)      // (the sequence-classification head reads no class token)
        if (mask[i] == 0 && ids[i] == e->cfg.class_token_index) {
            glc_set_err("forward: a class token (<<LABEL>>) lies under attention_mask 0 (row " + std::to_string(i / S) + ", position " + std::to_string(i % S) + "): not supported");
            return -1;
        }
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHK(hipSetDevice(e->device), -1);
    std::vector<int> cnt(B);
    std::vector<int> order, cuts;
    if (e->max_buckets > 1 && B > 1 && !e->keep_hidden) {
        // a row's effective length: one past its last attended token or class token
        std::vector<int> len(B, 0);
        for (int b = 0; b < B; ++b) {
            const int64_t* mk = mask + (size_t)b * S;
            const int64_t* id = ids + (size_t)b * S;
            int l = 0;
            for (int s = S - 1; s >= 0; --s) if (mk[s] != 0 || id[s] == e->cfg.class_token_index) { l = s + 1; break; }
            len[b] = l;
        }
        plan_buckets(len, e->max_buckets, BucketCost(e->cfg.hidden), order, cuts);
        if (cuts.size() > 2) {
            std::vector<int64_t> gi, gm;
            std::vector<float> gl;
            int lg = 2;      // glc_debug_last_forward_graph: the minimum over the groups
            // (graph replay: size the workspace for every group before the first one runs — a buffer that a later group moves would drop the
            //  graphs and the warmed-up keys of the groups ahead of it)
            if (e->graph_on)
                for (size_t g = 0; g + 1 < cuts.size(); ++g)
                    if (!ensure_capacity(e, cuts[g + 1] - cuts[g], std::max(len[order[cuts[g]]], 1), c_alloc)) return -1;
            for (size_t g = 0; g + 1 < cuts.size(); ++g) {
                const int i0 = cuts[g], n = cuts[g + 1] - cuts[g];
                int Sg = len[order[i0]];
                Sg = Sg < 1 ? 1 : Sg;
                gi.assign((size_t)n * Sg, 0); gm.assign((size_t)n * Sg, 0); gl.assign((size_t)n * (c_alloc > 0 ? c_alloc : 1), 0.f);
                for (int r = 0; r < n; ++r) {
                    memcpy(gi.data() + (size_t)r * Sg, ids + (size_t)order[i0 + r] * S, (size_t)Sg * sizeof(int64_t));
                    memcpy(gm.data() + (size_t)r * Sg, mask + (size_t)order[i0 + r] * S, (size_t)Sg * sizeof(int64_t));
                }
                std::vector<int> gc(n);
                if (forward_one(e, gi.data(), gm.data(), n, Sg, gl.data(), c_alloc, gc.data()) != 0) return -1;
                lg = e->last_graph < lg ? e->last_graph : lg;
                for (int r = 0; r < n; ++r) {
                    cnt[order[i0 + r]] = gc[r];
                    if (c_alloc > 0) memcpy(logits + (size_t)order[i0 + r] * c_alloc, gl.data() + (size_t)r * c_alloc, (size_t)c_alloc * sizeof(float));
                }
            }
            int cmax = 0;
            for (int b = 0; b < B; ++b) cmax = cnt[b] > cmax ? cnt[b] : cmax;
            if (c_out) *c_out = cmax;
            if (seqcls) finish();
            e->last_groups = (int)cuts.size() - 1;
            e->last_graph = lg;
            return 0;
        }
    }
    e->last_groups = 1;
    if (forward_one(e, ids, mask, B, S, logits, c_alloc, cnt.data()) != 0) return -1;
    int cmax = 0;
    for (int b = 0; b < B; ++b) cmax = cnt[b] > cmax ? cnt[b] : cmax;
    if (c_out) *c_out = cmax;
    if (seqcls) finish();
    return 0;
}

int glc_plan_length_buckets(const int* lengths, int B, int max_groups, int hidden, int* order, int* cuts, int* n_groups) {
    if (!lengths || B <= 0 || hidden <= 0 || !order || !cuts || !n_groups) { glc_set_err("plan_length_buckets: bad args"); return -1; }
    std::vector<int> len(lengths, lengths + B), ord, cu;
    plan_buckets(len, max_groups, BucketCost(hidden), ord, cu);
    for (int i = 0; i < B; ++i) order[i] = ord[i];
    for (size_t i = 0; i < cu.size(); ++i) cuts[i] = cu[i];
    *n_groups = (int)cu.size() - 1;
    return 0;
}

int glc_debug_last_forward_groups(const glc_engine* e) { return e ? e->last_groups : -1; }
int glc_debug_range_retries(const glc_engine* e) { return e ? e->range_retries : -1; }
int glc_debug_fp8_range_retries(const glc_engine* e) { return e ? e->fp8_retries : -1; }
int glc_debug_fp8_range_sticky(const glc_engine* e) { return e ? (e->fp8_sticky_off ? 1 : 0) : -1; }
int glc_debug_activation_exponent(const glc_engine* e) { return e ? e->act_sc : 1; }
long long glc_debug_mx_weight_bytes(const glc_engine* e) { return e ? (long long)e->mx_bytes : -1; }

int glc_engine_set_length_buckets(glc_engine* e, int max_groups) {
    if (!e || max_groups < 1 || max_groups > 64) { glc_set_err("set_length_buckets: 1..64 groups"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    graph_clear(e);
    e->max_buckets = max_groups;
    return 0;
}

int glc_engine_forward_device(glc_engine* e, const void* d_ids, const void* d_mask, int B, int S, int C, void* d_logits) {
    if (!e || !d_ids || !d_mask || (!d_logits && C > 0)) { glc_set_err("forward_device: null argument"); return -1; }
    if (!check_shape(e, B, S, C)) return -1;
    if (e->cfg.head_kind == GLC_HEAD_SEQCLS && C != e->cfg.cls_labels) {
        glc_set_err("forward_device: this engine has a sequence-classification head with " + std::to_string(e->cfg.cls_labels) + " labels: C = " + std::to_string(C) + " must equal cls_labels");
        return -1;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHK(hipSetDevice(e->device), -1);
    if (!ensure_capacity(e, B, S, C)) return -1;
    const bool mx_saved = e->mx;
    if (e->fp8_sticky_off) e->mx = false;
    const bool ok = graph_forward(e, (const int64_t*)d_ids, (const int64_t*)d_mask, B, S, C, (float*)d_logits);
    e->mx = mx_saved;
    if (!ok) return -1;
    // fp8 range guard (forward_one): a device-resident forward cannot be repeated behind the caller's back — the counter travels to a pinned
    // slot behind it, and glc_engine_sync reports a forward that left the range (and moves the engine to the split arithmetic)
    if (e->last_mx) { HIPCHK(hipMemcpyAsync(e->h_gxsat, e->d_gxsat, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, e->stream), -1); e->fp8_device_pending = true; }
    return 0;
}

/* Zero-shot NLI reduction over pair logits (include/gliclass_hip.h) */
int glc_engine_nli_scores(glc_engine* e, const float* d_logits, int T, int Lb, int entail_id, int contra_id, int multi_label, float* d_probs) {
    if (!e) { glc_set_err("nli_scores: null engine"); return -1; }
    if (!d_logits || !d_probs) { glc_set_err("nli_scores: null argument"); return -1; }
    if (e->cfg.head_kind != GLC_HEAD_SEQCLS) { glc_set_err("nli_scores: this engine has the GLiClass head; NLI scores need a sequence-classification head (head_kind = 1)"); return -1; }
    if (e->cfg.cls_labels < 2) { glc_set_err("nli_scores: the head has " + std::to_string(e->cfg.cls_labels) + " label; entailment and contradiction need cls_labels >= 2"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHK(hipSetDevice(e->device), -1);
    KCHK(glc_launch_nli_scores(e->stream, d_logits, T, Lb, e->cfg.cls_labels, entail_id, contra_id, multi_label, d_probs), -1);
    HIPCHK(hipGetLastError(), -1);
    return 0;
}

int glc_engine_sync(glc_engine* e) {
    if (!e) { glc_set_err("sync: null engine"); return -1; }
    HIPCHK(hipSetDevice(e->device), -1);
    HIPCHK(hipStreamSynchronize(e->stream), -1);
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->profile) prof_collect(e);
    if (e->fp8_device_pending) settle_device_range_check(e);
    if (e->device_invalid) {
        const int what = e->device_invalid;
        e->device_invalid = 0;
        if (what == 1)
            glc_set_err("sync: a device-resident forward since the last sync had activations beyond the fp8 range of the MX operand images (|x| > 448): its logits are "
                    "not valid; this engine's activation rows now carry exponent -5 (|x| up to 14336) — run the forward again");
        else
            glc_set_err("sync: a device-resident forward since the last sync had activations beyond the fp8 range of the MX operand images: its logits are "
                    "not valid; this engine now runs the split-f16 arithmetic (as GLICLASS_MX=0) — run the forward again");
        return -1;
    }
    return 0;
}

/* For callers of glc_engine_forward_device that wait for the engine's stream by other means than glc_engine_sync (hipStreamSynchronize,
 * an event, a consumer queued on the stream is NOT enough: it reads the logits before anybody has looked at the counter): once the stream's
 * work is complete, 1 = the logits of every device-resident forward since the last check are valid, 0 = one of them left the fp8 range of
 * the MX operand images — its logits are not valid (NaN-poisoned operand images), the engine has changed its arithmetic as glc_engine_sync
 * would have, run it again; -1 = error.  The stream must be idle: this call does not wait. */
int glc_engine_device_forward_valid(glc_engine* e) {
    if (!e) { glc_set_err("device_forward_valid: null engine"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    if (hipStreamQuery(e->stream) != hipSuccess) { glc_set_err("device_forward_valid: the engine's stream still has work queued — wait for it first (or call glc_engine_sync)"); return -1; }
    if (e->fp8_device_pending) settle_device_range_check(e);
    const int bad = e->device_invalid;
    e->device_invalid = 0;
    return bad ? 0 : 1;
}

void* glc_device_malloc(glc_engine* e, size_t bytes) {
    if (!e) { glc_set_err("device_malloc: null engine"); return nullptr; }
    if (hipSetDevice(e->device) != hipSuccess) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { glc_set_err("device_malloc failed"); return nullptr; }
    return p;
}
void glc_device_free(glc_engine* e, void* p) { if (e && p) { (void)hipSetDevice(e->device); (void)hipFree(p); } }
int glc_memcpy_h2d(glc_engine* e, void* dst, const void* src, size_t bytes) {
    if (!e) return -1;
    HIPCHK(hipSetDevice(e->device), -1);
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), -1);
    return 0;
}
int glc_memcpy_d2h(glc_engine* e, void* dst, const void* src, size_t bytes) {
    if (!e) return -1;
    HIPCHK(hipSetDevice(e->device), -1);
    HIPCHK(hipStreamSynchronize(e->stream), -1);
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), -1);
    return 0;
}

int glc_timer_start(glc_engine* e) {
    if (!e) return -1;
    HIPCHK(hipSetDevice(e->device), -1);
    HIPCHK(hipEventRecord(e->t0, e->stream), -1);
    return 0;
}
float glc_timer_stop_ms(glc_engine* e) {
    if (!e) return -1.f;
    HIPCHK(hipSetDevice(e->device), -1.f);
    HIPCHK(hipEventRecord(e->t1, e->stream), -1.f);
    HIPCHK(hipEventSynchronize(e->t1), -1.f);
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e->t0, e->t1), -1.f);
    return ms;
}

int glc_profile_enable(glc_engine* e, int on) {
    if (!e) return -1;
    std::lock_guard<std::mutex> lk(e->mu);
    graph_clear(e);
    e->profile = on != 0;
    e->ev_used = 0;
    for (int i = 0; i < PC_N; ++i) { e->prof_ms[i] = 0.f; e->prof_n[i] = 0; }
    return 0;
}
int glc_profile_read(glc_engine* e, const char** names, float* total_ms, int* launches, int max_n) {
    if (!e) return -1;
    std::lock_guard<std::mutex> lk(e->mu);
    int n = PC_N < max_n ? PC_N : max_n;
    for (int i = 0; i < n; ++i) { if (names) names[i] = kProfNames[i]; if (total_ms) total_ms[i] = e->prof_ms[i]; if (launches) launches[i] = e->prof_n[i]; }
    return n;
}

int glc_debug_set_group_split(glc_engine* e, int mode) {
    if (!e || mode < 0 || mode > 2) { glc_set_err("group_split: 0 off, 1 auto, 2 whenever the shapes allow"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    graph_clear(e);
    e->gs_mode = mode;
    return 0;
}
int glc_debug_last_forward_group_split(const glc_engine* e) { return e ? (e->last_gs ? 1 : 0) : -1; }
/* MX cross-term pipeline on / off (needs the GX weight copies: an engine created under GLICLASS_MX=1 or =build). */
int glc_debug_set_mx(glc_engine* e, int on) {
    if (!e) return -1;
    if (on && !e->mx_built) { glc_set_err("set_mx: the MX pipeline is not available to this engine (shapes, dtype, or GLICLASS_MX=0 at creation)"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    graph_clear(e);
    e->mx = on != 0;
    if (on) { e->fp8_sticky_off = false; e->fp8_streak = 0; e->act_sc = 0; }      // (a developer switching MX back on also clears the range guard's verdict)
    return 0;
}
int glc_debug_last_forward_mx(const glc_engine* e) { return e ? (e->last_mx ? 1 : 0) : -1; }
int glc_debug_last_forward_mx_attention(const glc_engine* e) { return e ? (e->last_mx && e->last_mx_attn ? 1 : 0) : -1; }
int glc_debug_last_forward_rope_epilogue(const glc_engine* e) { return e ? (e->last_mx && e->last_mx_attn && e->last_rope_epi ? 1 : 0) : -1; }
/* MX pipeline: attention on MX tiles (1, default) or on split-f16 units (0). */
int glc_debug_set_mx_attention(glc_engine* e, int on) { if (!e) return -1; std::lock_guard<std::mutex> lk(e->mu); graph_clear(e); e->mx_attn = on != 0; return 0; }
/* Developer: stop the next forwards after stage 10 * layer + k (k = 0 QKV, 1 attention, 2 attention-output, 3 FFN1, 4 FFN2 + LayerNorm;
 * -1 = run to the end; logits are garbage when stopped); glc_debug_read_workspace (engine_debug.hip) then reads the workspace rows. */
int glc_debug_set_stop(glc_engine* e, int stage) { if (!e) return -1; std::lock_guard<std::mutex> lk(e->mu); graph_clear(e); e->debug_stop = stage; return 0; }
/* Group-split pipeline with LayerNorm folded into the GEMMs (1, default) or as kernels of its own (0).  The folded weights are built
 * at load unless GLC_LNF=0 was set then; without them the switch has no effect. */
int glc_debug_last_forward_ln_folded(const glc_engine* e) { return e ? (e->last_lnf ? 1 : 0) : -1; }
int glc_debug_set_ln_fused(glc_engine* e, int on) {
    if (!e) return -1;
    std::lock_guard<std::mutex> lk(e->mu);
    graph_clear(e);
    e->ln_fused = on != 0;
    return 0;
}
/* Precision budget (developer): round operand groups of the default mode's group-split pipeline to f16 (PM_* bits of glc_kernels.h). */
int glc_debug_set_precision_mask(glc_engine* e, int mask) {
    if (!e || mask < 0 || mask >= (1 << 15)) { glc_set_err("precision_mask: 15 bits"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    graph_clear(e);
    e->prec_mask = mask;
    return 0;
}
/* 256-tile GEMM: full-line ring stages on / off, process-wide (developer A/B switch; results are bit-identical either way). */
int glc_debug_set_gemm_full_lines(int on) { glc_gemm_set_full_lines(on); return 0; }
int glc_debug_keep_hidden(glc_engine* e, int on) { if (!e) return -1; std::lock_guard<std::mutex> lk(e->mu); graph_clear(e); e->keep_hidden = on != 0; return 0; }
int glc_engine_set_prune_last_layer(glc_engine* e, int on) { if (!e) return -1; std::lock_guard<std::mutex> lk(e->mu); graph_clear(e); e->prune_last = on != 0; return 0; }
int glc_debug_last_forward_pruned(const glc_engine* e) { return e ? (e->last_pruned ? 1 : 0) : -1; }
int glc_debug_set_attention_impl(glc_engine* e, int impl) {
    if (!e || impl < 0 || impl > 3) { glc_set_err("bad attention impl"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    graph_clear(e);
    e->attn_impl = impl;
    return 0;
}

/* Captured-graph replay of forwards (include/gliclass_hip.h; graph_forward above).  Off drops every cached graph. */
int glc_engine_set_graph_replay(glc_engine* e, int on) {
    if (!e) { glc_set_err("set_graph_replay: null engine"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    graph_clear(e);
    e->graph_on = on != 0;
    return 0;
}
int glc_debug_last_forward_graph(const glc_engine* e) { return e ? e->last_graph : -1; }

/* MX pipeline for forwards below the 256 tile's fill rule, on the 128 tile of gemm128x.hip (include/gliclass_hip.h).  DeBERTa backbone only. */
int glc_engine_set_mx_small_forwards(glc_engine* e, int mode) {
    if (!e) { glc_set_err("set_mx_small_forwards: null engine"); return -1; }
    if (mode < 0 || mode > 2) { glc_set_err("set_mx_small_forwards: 0 off, 1 auto, 2 whenever the shapes allow"); return -1; }
    if (mode > 0 && e->cfg.backbone != GLC_BACKBONE_DEBERTA) {
        glc_set_err(std::string("set_mx_small_forwards: the 128 tile has no epilogue of the ") +
                    (e->cfg.backbone == GLC_BACKBONE_DECODER ? "decoder" : e->cfg.backbone == GLC_BACKBONE_BERT ? "bert" : e->cfg.backbone == GLC_BACKBONE_T5 ? "t5" : "modernbert") + " backbone (DeBERTa engines only)");
        return -1;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    graph_clear(e);
    e->mx_small = mode;
    return 0;
}
int glc_debug_last_forward_mx128(const glc_engine* e) { return e ? e->last_mx128 : -1; }
int glc_debug_graph_cache_size(const glc_engine* e) { return e ? graph_count(e) : -1; }

const glc_model_config* glc_engine_config(const glc_engine* e) { return e ? &e->cfg : nullptr; }
int glc_engine_dtype(const glc_engine* e) { return e ? e->dtype : -1; }

}  // extern "C"
