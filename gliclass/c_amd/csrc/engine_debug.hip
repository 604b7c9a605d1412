// Developer entries of include/gliclass_hip.h that allocate device buffers of their own or launch kernels outside a forward: the GEMM and
// attention microbenchmarks, the kernel-test entries (glc_debug_gemm_run, glc_debug_ln_stats_run) and the workspace read-back.  None of
// them runs in a forward; the one-line switches and counters that forwards read are in engine.hip.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "engine_internal.h"

namespace {
// device buffers of one call of an entry in this file (freed when it returns)
struct RunBufs {
    std::vector<void*> v;
    ~RunBufs() { for (void* p : v) (void)hipFree(p); }
    void* get(size_t bytes) { void* p = nullptr; if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr; v.push_back(p); return p; }
    void* up(const void* h, size_t bytes) { void* p = get(bytes); if (p && hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr; return p; }
};
// One launch of a stamped kernel build: `launch` gets n zeroed 64-bit counters in device memory, hs their values once the stream has drained.
// false = nothing to print: no buffer, no read-back, or the launcher refused (its message goes to stderr under `tag`).
template <class Launch> bool run_stamped(hipStream_t st, const char* tag, size_t n, std::vector<unsigned long long>& hs, Launch launch) {
    RunBufs bufs;
    unsigned long long* d = (unsigned long long*)bufs.get(n * sizeof(unsigned long long));
    if (!d) return false;
    (void)hipMemsetAsync(d, 0, n * sizeof(unsigned long long), st);
    const char* m = launch(d);
    (void)hipStreamSynchronize(st);
    if (m) { fprintf(stderr, "[%s] %s\n", tag, m); return false; }
    hs.resize(n);
    return hipMemcpy(hs.data(), d, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess;
}
// ... and its counters summed over the records: hs = [records][per] -> [per]
std::vector<double> stamp_sums(const std::vector<unsigned long long>& hs, size_t per) {
    std::vector<double> s(per, 0.0);
    for (size_t i = 0; i < hs.size(); ++i) s[i % per] += (double)hs[i];
    return s;
}
constexpr size_t RUN_GUARD = 1u << 20;     // bytes of guard before and after every output
// bytes of output i (C, or Qh / Kh / Vt) the launch may write; 0 = that output does not exist (or the shape is one every launcher refuses)
size_t gemm_run_out_bytes(const glc_gemm_run& r, int dtype, int i) {
    const bool wide = r.kernel == GLC_GEMM_RUN_GS || r.kernel == GLC_GEMM_RUN_MX || r.kernel == GLC_GEMM_RUN_MX128;       // GS / GX rows, split units, MX tiles and plain fp32: 4 bytes per element
    const size_t es = wide ? 4 : esize(dtype);
    if (r.epi == EPI_QKV || r.epi == EPI_QKVR) {
        if (r.Sp <= 0 || r.Mvalid <= 0) return 0;
        const size_t rows = (size_t)std::min(r.Mvalid, r.Mpad), B = (rows + r.Sp - 1) / r.Sp;
        if (r.epi == EPI_QKVR) return r.nq > 0 && r.nkv > 0 ? B * (size_t)(i == 0 ? r.nq : r.nkv) * r.Sp * 128 * 4 : 0;
        return r.nh > 0 ? B * (size_t)r.nh * r.Sp * 64 * es : 0;
    }
    if (i > 0) return 0;
    const bool glu = r.epi == EPI_SWIGLU || r.epi == EPI_GEGLU;
    return (size_t)r.Mpad * (size_t)(glu ? r.N / 2 : r.N) * es;
}
}  // namespace
extern "C" {

/* Workspace rows as fp32, usually of a forward stopped by glc_debug_set_stop: which = 0 X, 1 H1, 2 CTX, 3 FF (row formats decoded: GX
 * after an MX forward, GS after a group-split one), 4 T1 (plain fp32), 5 statsA, 6 statsB (2 floats per row), 7 Qh, 8 Kh, 9 Vt (raw units). */
int glc_debug_read_workspace(glc_engine* e, int which, int rows, float* out) {
    if (!e || !out || rows <= 0 || which < 0 || which > 9) { glc_set_err("read_workspace: bad args"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHK(hipSetDevice(e->device), -1);
    HIPCHK(hipStreamSynchronize(e->stream), -1);
    if (rows > e->capM) { glc_set_err("read_workspace: more rows than the workspace holds"); return -1; }
    const int H = e->cfg.hidden, I = e->cfg.inter;
    if (which >= 7) { HIPCHK(hipMemcpy(out, which == 7 ? e->Qh : which == 8 ? e->Kh : e->Vt, (size_t)rows * e->cfg.hidden * 4, hipMemcpyDeviceToHost), -1); return 0; }   // raw units
    if (which >= 5) { HIPCHK(hipMemcpy(out, which == 5 ? e->statsA : e->statsB, (size_t)rows * 8, hipMemcpyDeviceToHost), -1); return 0; }
    const void* src = which == 0 ? e->X : which == 1 ? e->H1 : which == 2 ? e->CTX : which == 3 ? e->FF : e->T1;
    const int W = which == 3 ? I : H;
    std::vector<unsigned char> raw((size_t)rows * W * 4);
    HIPCHK(hipMemcpy(raw.data(), src, raw.size(), hipMemcpyDeviceToHost), -1);
    if (which == 4 || !e->last_gs) { memcpy(out, raw.data(), raw.size()); return 0; }
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < W; ++c) {
            const unsigned char* g = raw.data() + ((size_t)r * W + (c & ~31)) * 4;
            _Float16 hi, lo; memcpy(&hi, g + 2 * (c & 31), 2);
            float v = (float)hi;
            if (e->last_mx) {
                const unsigned char b = g[64 + 16 * ((c & 31) >> 3) + (c & 7)];
                const int sg = b >> 7, ex = (b >> 3) & 15, mn = b & 7;
                const float l8 = ex == 0 ? ldexpf((float)mn, -9) : ldexpf(1.0f + mn / 8.0f, ex - 7);
                v += (sg ? -l8 : l8) * ldexpf(1.0f, -GLC_GX_SHIFT - e->act_sc);
            } else { memcpy(&lo, g + 64 + 2 * (c & 31), 2); v += (float)lo; }
            out[(size_t)r * W + c] = v;
        }
    return 0;
}

int glc_debug_read_pos_ids(glc_engine* e, int32_t* out, int n) {
    if (!e || !out || n <= 0) { glc_set_err("read_pos_ids: bad args"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->cfg.backbone != GLC_BACKBONE_BERT || !e->pos_ids || n != e->lastB * e->lastSp) { glc_set_err("read_pos_ids: a BERT engine's last forward has B * Sp ids"); return -1; }
    HIPCHK(hipSetDevice(e->device), -1);
    HIPCHK(hipStreamSynchronize(e->stream), -1);
    HIPCHK(hipMemcpy(out, e->pos_ids, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost), -1);
    return 0;
}

int glc_debug_get_hidden(glc_engine* e, int which, float* out, size_t out_elems) {
    if (!e || !out) { glc_set_err("get_hidden: null"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    const int B = e->lastB, S = e->lastS, Sp = e->lastSp, H = e->cfg.hidden;
    if (!e->hidden_dump || B == 0 || which < 0 || which > e->cfg.layers) { glc_set_err("get_hidden: nothing recorded"); return -1; }
    if (out_elems < (size_t)B * S * H) { glc_set_err("get_hidden: output too small"); return -1; }
    HIPCHK(hipSetDevice(e->device), -1);
    const size_t M = (size_t)B * Sp, es = esize(e->dtype);
    float* tmp = nullptr;
    HIPCHK(hipMalloc((void**)&tmp, M * H * sizeof(float)), -1);
    const char* m = glc_launch_to_f32(e->stream, e->dtype, (char*)e->hidden_dump + (size_t)which * M * H * es, tmp, M * H);
    if (m) { (void)hipFree(tmp); glc_set_err(m); return -1; }
    hipError_t r = hipMemcpy2DAsync(out, (size_t)S * H * sizeof(float), tmp, (size_t)Sp * H * sizeof(float), (size_t)S * H * sizeof(float), B,
                                    hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    (void)hipFree(tmp);
    if (r != hipSuccess) { glc_set_err(std::string("get_hidden: ") + hipGetErrorString(r)); return -1; }
    return 0;
}

/* Developer microbenchmark: time `iters` launches of one GEMM shape on random 16-bit data (HIP events).
 * which: 0 = auto (256-tile when possible), 1 = force the 128x128 kernel.  Returns ms per launch or <0. */
float glc_debug_gemm_bench(glc_engine* e, int M, int N, int K, int epi, int iters, int which) {
    // which == 6: the group-split fp32-mode kernel (rows of [32 hi | 32 lo] f16 groups, 4 bytes per element; any engine dtype)
    const int which_in = which;
    if (which >= 100) which %= 100;
    const bool mxb = which == 9;                      // the MX cross-term kernel on GX rows (gemm256x.hip); which = 100 (1 + prio) + 9: wave priority policy prio
    const bool gsb = which == 6 || which == 8 || mxb;
    const int mx_ws = glc_gx_weight_exponent(0.5f);
    if (!e || M <= 0 || N <= 0 || K <= 0 || iters <= 0 || which_in >= 1000 || (which >= 10 && which <= 14) || (e->dtype == GLC_F32 && !gsb) || epi < EPI_BIAS || epi > EPI_RESID) {
        glc_set_err("gemm_bench: bad args"); return -1.f;
    }
    if (M % 256 || N % 256 || K % 64) { glc_set_err("gemm_bench: M,N %256, K %64 required"); return -1.f; }
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHK(hipSetDevice(e->device), -1.f);
    const size_t es = gsb ? 4 : 2;
    const size_t nA = (size_t)M * K, nW = (size_t)N * K, nC = (size_t)M * N;
    const size_t nmax = nA > nW ? (nA > nC ? nA : nC) : (nW > nC ? nW : nC);
    RunBufs bufs;
    void *A = bufs.get(nA * es), *W = bufs.get(nW * es), *C = bufs.get(nC * es), *R = bufs.get(nC * es);
    float *bias = (float*)bufs.get(N * sizeof(float)), *tmp = (float*)bufs.get(nmax * sizeof(float));
    if (!A || !W || !C || !R || !bias || !tmp) { glc_set_err("gemm_bench: alloc failed"); return -1.f; }
    std::vector<float> h(nmax);
    unsigned s = 12345u;
    const char* zenv = glc_dev_env("GLC_BENCH_DATA");       // developer: "zero" = all-zero operands, "const" = one value everywhere (how much of the time is the power envelope?)
    for (size_t i = 0; i < nmax; ++i) { s = s * 1664525u + 1013904223u; h[i] = zenv && zenv[0] == 'z' ? 0.f : zenv && zenv[0] == 'c' ? 0.37f : ((float)(s >> 8) / 8388608.f - 1.f) * 0.5f; }
    if (hipMemcpy(tmp, h.data(), nmax * sizeof(float), hipMemcpyHostToDevice)) { glc_set_err("gemm_bench: copy failed"); return -1.f; }
    if (gsb) {      // fp32 values, split in place into the group-split image (or the GX image)
        if (hipMemcpyAsync(A, tmp, nA * 4, hipMemcpyDeviceToDevice, e->stream) || hipMemcpyAsync(W, tmp, nW * 4, hipMemcpyDeviceToDevice, e->stream) ||
            hipMemcpyAsync(R, tmp, nC * 4, hipMemcpyDeviceToDevice, e->stream)) { glc_set_err("gemm_bench: copy failed"); return -1.f; }
        if (mxb ? (glc_launch_to_gx(e->stream, A, nA, 0, 0) || glc_launch_to_gx(e->stream, W, nW, mx_ws, 1) || glc_launch_to_gx(e->stream, R, nC, 0, 0))
                : (glc_launch_presplit(e->stream, A, nA) || glc_launch_presplit(e->stream, W, nW) || glc_launch_presplit(e->stream, R, nC))) { glc_set_err("gemm_bench: split failed"); return -1.f; }
    } else if (glc_launch_convert(e->stream, e->dtype, tmp, A, nA) || glc_launch_convert(e->stream, e->dtype, tmp, W, nW) ||
               glc_launch_convert(e->stream, e->dtype, tmp, R, nC)) { glc_set_err("gemm_bench: convert failed"); return -1.f; }
    if (hipMemcpyAsync(bias, tmp, N * sizeof(float), hipMemcpyDeviceToDevice, e->stream)) return -1.f;
    GemmArgs g; g.A = A; g.W = W; g.bias = bias; g.C = C; g.resid = R; g.Mpad = M; g.N = N; g.K = K; g.mx_ws = mx_ws;
    if (mxb && which_in >= 100) g.prio_mode = which_in / 100 - 1;      // which = 100 (1 + prio) + 9
    const char* m = nullptr;
    auto launch = [&]() -> const char* { return mxb ? glc_launch_gemm256x(e->stream, epi, g) : gsb ? glc_launch_gemm256s_gs(e->stream, epi, g) : which == 1 ? glc_launch_gemm(e->stream, e->dtype, epi, g) : (which == 5 || which == 7) ? glc_launch_gemm256s(e->stream, e->dtype, epi, g) : glc_launch_gemm_auto(e->stream, e->dtype, epi, g); };
    for (int i = 0; i < 2 && !m; ++i) m = launch();
    if (m) { glc_set_err(m); return -1.f; }
    if (hipEventRecord(e->t0, e->stream)) return -1.f;
    for (int i = 0; i < iters; ++i) launch();
    if (hipEventRecord(e->t1, e->stream) || hipEventSynchronize(e->t1)) { glc_set_err("gemm_bench: sync failed"); return -1.f; }
    float t = 0.f;
    if (hipEventElapsedTime(&t, e->t0, e->t1)) return -1.f;
    std::vector<unsigned long long> hs;
    // diagnostic: one stamped launch of the full-line 256-tile kernel (7: 16-bit operands, 8: group-split), EPI_BIAS: 64 workgroups x 8 waves x 12 counters, then (entry, exit) pairs
    if ((which == 7 || which == 8) && run_stamped(e->stream, "gemm256s stamps", 64 * 8 * 14, hs, [&](unsigned long long* d) {
            GemmArgs gd = g; gd.stamps = d;
            return which == 8 ? glc_launch_gemm256s_gs(e->stream, EPI_BIAS, gd) : glc_launch_gemm256s(e->stream, e->dtype, EPI_BIAS, gd);
        })) {
        for (int grp = 0; grp < 2; ++grp) {       // wave group 0 (waves 0-3) / the late group (waves 4-7)
            double sg[12] = {0};
            for (int b = 0; b < 64; ++b) for (int w = 4 * grp; w < 4 * grp + 4; ++w) for (int k = 0; k < 12; ++k) sg[k] += (double)hs[((size_t)b * 8 + w) * 12 + k];
            const double n = 64 * 4, ng = sg[11] / n > 0 ? sg[11] / n : 1;
            fprintf(stderr, "[gemm256s stamps M=%d N=%d K=%d %s, waves %d-%d] cycles per group and wave: E: dma %.0f reads+wait %.0f barrier %.0f mfma %.0f barrier %.0f | "
                            "O: (dma %.0f) reads+wait %.0f barrier %.0f mfma %.0f barrier %.0f | total %.0f | clock %.0f MHz\n", M, N, K, which == 8 ? "group-split" : "16-bit", 4 * grp, 4 * grp + 3,
                    sg[0] / n / ng, sg[1] / n / ng, sg[2] / n / ng, sg[3] / n / ng, sg[4] / n / ng, sg[5] / n / ng, sg[6] / n / ng, sg[7] / n / ng, sg[8] / n / ng, sg[9] / n / ng,
                    (sg[0] + sg[1] + sg[2] + sg[3] + sg[4] + sg[5] + sg[6] + sg[7] + sg[8] + sg[9]) / n / ng, sg[10] / n / 10.0);
        }
        double pro = 0, epi = 0;
        for (size_t i = 0; i < 64 * 8; ++i) { pro += (double)hs[64 * 8 * 12 + 2 * i]; epi += (double)hs[64 * 8 * 12 + 2 * i + 1]; }
        fprintf(stderr, "[gemm256s stamps] per tile and wave: entry -> loop %.0f cycles, loop end -> stores retired %.0f cycles\n", pro / (64 * 8), epi / (64 * 8));
    }
    return t / iters;
}

/* Kernel-level tests: one launcher call on caller-supplied operands, raw bytes back (include/gliclass_hip.h). */
int glc_debug_gemm_run(glc_engine* e, glc_gemm_run* r) {
    if (!e || !r || r->kernel < GLC_GEMM_RUN_128 || r->kernel > GLC_GEMM_RUN_MX128 || r->epi < EPI_BIAS || r->epi > EPI_GEGLU || r->Mpad <= 0 || r->N <= 0 || r->K <= 0 ||
        r->Mpad > (1 << 20) || r->N > (1 << 20) || r->K > (1 << 20) || !r->A || !r->W || (r->W2 && r->kernel != GLC_GEMM_RUN_128) || r->ws_bytes > (1ull << 30)) {
        glc_set_err("gemm_run: bad args"); return -1;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHK(hipSetDevice(e->device), -1);
    const int dtype = e->dtype, kern = r->kernel;
    const bool gs = kern == GLC_GEMM_RUN_GS, mx = kern == GLC_GEMM_RUN_MX || kern == GLC_GEMM_RUN_MX128;
    const size_t es = gs || mx ? 4 : esize(dtype);
    auto up32 = [](size_t n) { return (n + 31) / 32 * 32; };      // the group converters take whole 32-groups (a row length they cut wrongly is one the launcher refuses)
    const size_t nA = (size_t)r->Mpad * r->K, nW = (size_t)r->N * r->K, nC = (size_t)r->Mpad * r->N;
    RunBufs bufs;
    hipStream_t st = e->stream;
    const char* msg = nullptr;
    bool own = false;                               // msg is this entry's own failure (allocation, copy), not a refusal
    // fp32 host values -> the operand image this kernel reads; role: 0 = activation rows (A, resid), 1 = weight rows
    auto encode = [&](const float* h, size_t n, int role, bool plain) -> void* {
        const size_t n32 = up32(n);
        float* tmp = (float*)bufs.get(n32 * 4);
        if (!tmp || hipMemsetAsync(tmp, 0, n32 * 4, st) != hipSuccess || hipMemcpyAsync(tmp, h, n * 4, hipMemcpyHostToDevice, st) != hipSuccess) { msg = "gemm_run: operand upload failed"; own = true; return nullptr; }
        if (plain) return tmp;
        if (gs) { msg = glc_launch_presplit(st, tmp, n32); return msg ? nullptr : tmp; }
        if (mx) {
            if (role == 1 && r->w_from_gs) {        // the engine's path: the split-f16 copy first, the GX copy from it
                void* gx = bufs.get(n32 * 4);
                if (!gx) { msg = "gemm_run: alloc failed"; own = true; return nullptr; }
                msg = glc_launch_presplit(st, tmp, n32);
                if (!msg) msg = glc_launch_gs_to_gx(st, tmp, gx, n32, r->mx_ws);
                return msg ? nullptr : gx;
            }
            msg = glc_launch_to_gx(st, tmp, n32, role == 1 ? r->mx_ws : r->act_sc, role);
            return msg ? nullptr : tmp;
        }
        if (dtype == GLC_F32) {
            if (role == 1 && r->w_presplit) msg = glc_launch_presplit(st, tmp, n32);
            return msg ? nullptr : tmp;
        }
        void* img = bufs.get(n32 * 2);
        if (!img) { msg = "gemm_run: alloc failed"; own = true; return nullptr; }
        msg = glc_launch_convert(st, dtype, tmp, img, n);
        return msg ? nullptr : img;
    };
    auto fail = [&](const char* m, int rc) { (void)hipStreamSynchronize(st); glc_set_err(m); return rc; };
    GemmArgs g;
    g.Mpad = r->Mpad; g.N = r->N; g.K = r->K; g.m_split = r->m_split; g.Mvalid = r->Mvalid; g.Sp = r->Sp; g.nh = r->nh; g.H = r->H; g.nq = r->nq; g.nkv = r->nkv;
    g.qscale = r->qscale; g.qkv_skip_q = r->qkv_skip_q; g.qkv_split = r->qkv_split; g.qkv_mxt = r->qkv_mxt; g.gs_c_plain = r->gs_c_plain; g.gs_resid_plain = r->gs_resid_plain;
    g.perm_cols = r->perm_cols; g.glu_interleaved = r->glu_interleaved; g.prec = r->prec; g.mx_ws = r->mx_ws; g.act_sc = r->act_sc; g.gx_rows = r->gx_rows;
    g.w_presplit = kern == GLC_GEMM_RUN_128 && dtype == GLC_F32 && r->w_presplit;
    g.A = encode(r->A, nA, 0, false);
    if (!msg) g.W = encode(r->W, nW, 1, false);
    if (!msg && r->W2) g.W2 = encode(r->W2, nW, 1, false);
    if (!msg && r->resid) g.resid = encode(r->resid, nC, 0, (gs || mx) && r->gs_resid_plain);
    if (msg) return fail(msg, own ? -1 : -2);      // a converter's refusal counts as the launcher's: nothing has been launched
    auto upf = [&](const float* h, size_t n) -> const float* { if (!h) return nullptr; const float* p = (const float*)bufs.up(h, n * 4); if (!p) msg = "gemm_run: upload failed"; return p; };
    g.bias = upf(r->bias, r->N); g.bias2 = upf(r->bias2, r->N); g.ln_c = upf(r->ln_c, r->N); g.r_gamma = upf(r->r_gamma, r->N); g.r_beta = upf(r->r_beta, r->N);
    g.a_stats = (const float2*)upf(r->a_stats, 2 * (size_t)r->Mpad); g.r_stats = (const float2*)upf(r->r_stats, 2 * (size_t)r->Mpad);
    if (r->rope_cs) { if (r->Sp <= 0 || r->Sp > (1 << 16)) return fail("gemm_run: bad args", -1); g.rope_cs = upf(r->rope_cs, (size_t)r->Sp * 128); }
    if (r->q_tile_flag) {
        const size_t nf = (size_t)r->Mpad / 32 + 8;
        unsigned char* f = (unsigned char*)bufs.get(nf);
        if (!f || hipMemset(f, 0, nf) != hipSuccess || hipMemcpy(f, r->q_tile_flag, (size_t)r->Mpad / 32, hipMemcpyHostToDevice) != hipSuccess) msg = "gemm_run: upload failed";
        g.q_tile_flag = f;
    }
    if (r->ws_bytes) { g.ws = (float*)bufs.get(r->ws_bytes); g.ws_bytes = r->ws_bytes; if (!g.ws) msg = "gemm_run: alloc failed"; }
    if (msg) return fail(msg, -1);
    // outputs: [guard | bytes | guard], all prefilled
    struct Guarded { unsigned char* base = nullptr; size_t bytes = 0; };
    Guarded outs[4];
    const int fillb = r->fill & 255;
    auto guarded = [&](Guarded& o, size_t bytes) {
        o.bytes = bytes;
        o.base = (unsigned char*)bufs.get(bytes + 2 * RUN_GUARD);
        return o.base && hipMemsetAsync(o.base, fillb, bytes + 2 * RUN_GUARD, st) == hipSuccess;
    };
    for (int i = 0; i < 3; ++i) {
        const size_t need = gemm_run_out_bytes(*r, dtype, i);
        if (need > r->out_bytes[i]) return fail("gemm_run: out_bytes is smaller than the output this launch writes", -1);
        if (!guarded(outs[i], std::max<size_t>(need, 16))) return fail("gemm_run: alloc failed", -1);
    }
    const size_t lp_bytes = (size_t)r->Mpad * (size_t)(r->N / 64) * 8;
    if (r->want_ln_part) { if (!guarded(outs[3], std::max<size_t>(lp_bytes, 16))) return fail("gemm_run: alloc failed", -1); g.ln_part = (float2*)(outs[3].base + RUN_GUARD); }
    if (r->epi == EPI_QKV || r->epi == EPI_QKVR) { g.Qh = outs[0].base + RUN_GUARD; g.Kh = outs[1].base + RUN_GUARD; g.Vt = outs[2].base + RUN_GUARD; }
    else g.C = outs[0].base + RUN_GUARD;
    unsigned* sat = (unsigned*)bufs.get(8);
    if (!sat || hipMemsetAsync(sat, 0, 8, st) != hipSuccess) return fail("gemm_run: alloc failed", -1);
    if (mx) g.gx_sat = sat;
    // the one launcher call
    switch (kern) {
        case GLC_GEMM_RUN_128: msg = glc_launch_gemm(st, dtype, r->epi, g); break;
        case GLC_GEMM_RUN_256S: msg = glc_launch_gemm256s(st, dtype, r->epi, g); break;
        case GLC_GEMM_RUN_GS: msg = glc_launch_gemm256s_gs(st, r->epi, g); break;
        case GLC_GEMM_RUN_MX: msg = glc_launch_gemm256x(st, r->epi, g); break;
        case GLC_GEMM_RUN_MX128: msg = glc_launch_gemm128x(st, r->epi, g); break;
        default: msg = glc_launch_gemm_auto(st, dtype, r->epi, g); break;
    }
    if (msg) return fail(msg, -2);
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) { glc_set_err(std::string("gemm_run: ") + hipGetErrorString(he)); return -1; }
    auto back = [&](void* h, const void* d, size_t bytes) { return !h || !bytes || hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    bool ok = true;
    for (int i = 0; i < 3; ++i) ok = ok && back(r->out[i], outs[i].base + RUN_GUARD, gemm_run_out_bytes(*r, dtype, i));
    if (r->want_ln_part) ok = ok && back(r->ln_part, outs[3].base + RUN_GUARD, lp_bytes);
    ok = ok && back(r->A_img, g.A, nA * es) && back(r->W_img, g.W, nW * es) && (!g.W2 || back(r->W2_img, g.W2, nW * es)) &&
         (!g.resid || back(r->resid_img, g.resid, nC * ((gs || mx) && r->gs_resid_plain ? 4 : es))) && back(r->sat, sat, 8);
    std::vector<unsigned char> gd(RUN_GUARD);
    r->guards_ok = 1;
    r->cus = glc_device_cus();
    for (int i = 0; i < 4 && ok; ++i) {
        if (!outs[i].base) continue;
        for (int side = 0; side < 2 && ok; ++side) {
            ok = back(gd.data(), outs[i].base + (side ? RUN_GUARD + outs[i].bytes : 0), RUN_GUARD);
            for (size_t k = 0; k < RUN_GUARD && ok; ++k) if (gd[k] != (unsigned char)fillb) { r->guards_ok = 0; break; }
        }
    }
    if (!ok) { glc_set_err("gemm_run: readback failed"); return -1; }
    return 0;
}

int glc_debug_ln_stats_run(glc_engine* e, const float* part, int nparts, int M, float eps, int rms, float* stats) {
    if (!e || !part || !stats || M <= 0 || nparts <= 0 || M > (1 << 20) || nparts > 1024) { glc_set_err("ln_stats_run: bad args"); return -1; }
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHK(hipSetDevice(e->device), -1);
    RunBufs bufs;
    const float2* dp = (const float2*)bufs.up(part, (size_t)M * nparts * 8);
    float2* ds = (float2*)bufs.get((size_t)M * 8);
    if (!dp || !ds) { glc_set_err("ln_stats_run: alloc failed"); return -1; }
    KCHK(glc_launch_ln_stats(e->stream, dp, nparts, ds, M, nparts * 64, eps, rms), -2);
    HIPCHK(hipStreamSynchronize(e->stream), -1);
    HIPCHK(hipMemcpy(stats, ds, (size_t)M * 8, hipMemcpyDeviceToHost), -1);
    return 0;
}

/* Developer microbenchmark: re-run the band attention kernel `iters` times on the Q/K/V^T that the last forward left in the
 * workspace (layer-0 position tables), HIP-event timed.  checksum[0..1] = sum and sum of squares of the context output;
 * variant is passed through to the kernel; stamps != 0 adds one launch of the s_memtime-instrumented build and prints
 * the per-tile segment cycles.  Returns ms per launch or < 0. */
float glc_debug_attn_bench(glc_engine* e, int iters, int variant, int stamps, double* checksum) {
    if (!e || iters <= 0 || (e->dtype == GLC_F32 && !e->attn_split) || e->lastB <= 0 || e->cfg.backbone != GLC_BACKBONE_DEBERTA) {
        glc_set_err("attn_bench: needs a DeBERTa engine (16-bit, or fp32 with split-f16 attention) and a previous forward"); return -1.f;
    }
    constexpr int MX_DEV = 256 | 512 | 4096 | 16384 | 65536 | 131072 | 262144 | 1048576;     // the MX kernel's timing-only and measurement builds
    if (variant & ~(255 | 1024 | 2048 | MX_DEV)) { glc_set_err("attn_bench: no attention kernel takes these variant bits"); return -1.f; }
#ifndef GLC_DEVELOPER
    if (stamps || (variant & MX_DEV)) { glc_set_err("attn_bench: stamped and timing-only builds (wrong results) exist in developer builds only (make DEV=1)"); return -1.f; }
#endif
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHK(hipSetDevice(e->device), -1.f);
    const int B = e->lastB, Sp = e->lastSp, H = e->cfg.hidden, nh = e->cfg.heads;
    const LayerW& w = e->layers[0];
    const bool sp = e->dtype == GLC_F32;
    AttnArgs a{e->Qh, e->Kh, e->Vt, sp ? w.PKs : w.PK, sp ? w.PQs : w.PQ, e->dtabs[Sp], e->kbias, e->klen, e->kfirst, e->CTX, B, nh, Sp, H, e->P};
    a.rsat_pos = e->dsat[Sp].first; a.rsat_neg = e->dsat[Sp].second; a.variant = variant & 123; a.otab = e->otabs[Sp]; a.mtab = e->mtabs.count(Sp) ? e->mtabs[Sp] : nullptr; a.split = sp;    // bits 0-1: per-wave kernel diagnostics; bit 3: wg kernel without the K/V ring; bits 4 / 5: wg kernel with / without the half-tile stagger
    hipStream_t st = e->stream;
    const bool wg = (variant & 4) != 0;                       // bit 2: the workgroup-shared kernel (attention_wg.hip)
    const bool mxk = (variant & 128) != 0;                    // bit 7: the MX-tile kernel (attention_mx.hip) on the MX tiles the last (MX) forward left; bits 8 / 9: its timing-only builds
    if (mxk) {
        if (!(sp && e->last_mx && e->mx_attn && w.PKm && w.PQm)) { glc_set_err("attn_bench: the MX kernel needs a previous forward of the MX pipeline with MX attention"); return -1.f; }
        a.PK = w.PKm; a.PQ = w.PQm; a.ctx_gs = 2; a.variant = variant & (1024 | 2048 | MX_DEV);
    }
    auto launch = [&]() -> const char* { return mxk ? glc_launch_attention_mx(st, a) : wg ? glc_launch_attention_wg(st, e->dtype, a) : glc_launch_attention(st, e->dtype, 2, a); };
    for (int i = 0; i < 2; ++i) KCHK(launch(), -1.f);
    HIPCHK(hipEventRecord(e->t0, st), -1.f);
    for (int i = 0; i < iters; ++i) launch();
    HIPCHK(hipEventRecord(e->t1, st), -1.f);
    HIPCHK(hipEventSynchronize(e->t1), -1.f);
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, e->t0, e->t1), -1.f);
    if (checksum) {
        const size_t n = (size_t)B * Sp * H;
        float* tmp = nullptr;
        HIPCHK(hipMalloc((void**)&tmp, n * sizeof(float)), -1.f);
        std::vector<float> h(n);
        const char* m = mxk ? nullptr : glc_launch_to_f32(st, e->dtype, e->CTX, tmp, n);
        if (mxk) { HIPCHK(hipMemsetAsync(tmp, 0, n * sizeof(float), st), -1.f); }        // (GX rows: no checksum)
        hipError_t r = m ? hipErrorUnknown : hipMemcpyAsync(h.data(), tmp, n * sizeof(float), hipMemcpyDeviceToHost, st);
        if (r == hipSuccess) r = hipStreamSynchronize(st);
        (void)hipFree(tmp);
        if (r != hipSuccess) { glc_set_err("attn_bench: readback failed"); return -1.f; }
        double s1 = 0, s2 = 0;
        for (size_t i = 0; i < n; ++i) { s1 += h[i]; s2 += (double)h[i] * h[i]; }
        checksum[0] = s1; checksum[1] = s2;
    }
    // one launch of a stamped build: a record of counters per wave, the last one the wave's tile count
    std::vector<unsigned long long> hs;
    auto stamped = [&](const char* tag, size_t waves, size_t per, auto run) {
        return run_stamped(st, tag, waves * per, hs, [&](unsigned long long* d) { AttnArgs as = a; as.stamps = d; return run(as); });
    };
    if (stamps && wg && sp && !(variant & 121) &&      // the split-f16 workgroup kernel: 64 workgroups x 8 waves x 8 counters
        stamped("attn_wg stamps", 64 * 8, 8, [&](const AttnArgs& as) { return glc_launch_attention_wg(st, e->dtype, as); })) {
        const std::vector<double> s = stamp_sums(hs, 8);
        const double nt = s[7] > 0 ? s[7] : 1;
        fprintf(stderr, "[attn_wg stamps] per band tile per wave (s_memtime ticks), %.0f tiles: request wait %.0f | K+gather+p2c/S issue %.0f | barrier X %.0f | "
                        "image stores + barrier Y %.0f | DMA, image gather, c2p issue %.0f | softmax + P.V + c2p store %.0f | total %.0f | s_memtime clock %.0f MHz\n",
                nt, s[0] / nt, s[1] / nt, s[2] / nt, s[3] / nt, s[4] / nt, s[5] / nt, (s[0] + s[1] + s[2] + s[3] + s[4] + s[5]) / nt, s[6] / (64 * 8) / 10.0);
    }
    if (stamps && mxk &&                               // the MX-tile kernel: 64 workgroups x 8 waves x 10 counters
        stamped("attn_mx stamps", 64 * 8, 10, [&](const AttnArgs& as) { return glc_launch_attention_mx(st, as); })) {
        const std::vector<double> s = stamp_sums(hs, 10);
        const double nt = s[9] > 0 ? s[9] : 1;
        double tot = 0;
        for (int k = 0; k < 8; ++k) tot += s[k];
        fprintf(stderr, "[attn_mx stamps] per band tile per wave (s_memtime ticks), %.0f tiles: request wait %.0f | K + c2p gather + p2c/S issue %.0f | row requests %.0f | "
                        "barrier X %.0f | image stores + barrier Y %.0f | DMA + image gather %.0f | c2p issue + softmax + P.V %.0f | c2p store %.0f | total %.0f | s_memtime clock %.0f MHz\n",
                nt, s[0] / nt, s[1] / nt, s[2] / nt, s[3] / nt, s[4] / nt, s[5] / nt, s[6] / nt, s[7] / nt, tot / nt, s[8] / (64 * 8) / 10.0);
    }
    if (stamps && !wg && !sp &&                        // the per-wave 16-bit kernel: 64 workgroups x 4 waves x 8 counters (a refusal prints the zero counters)
        stamped("attn stamps", 64 * 4, 8, [&](const AttnArgs& as) { glc_launch_attention(st, e->dtype, 2, as); return (const char*)nullptr; })) {
        const std::vector<double> s = stamp_sums(hs, 8);
        const double nt = s[7] > 0 ? s[7] : 1;
        fprintf(stderr, "[attn stamps] per band tile per wave (s_memtime ticks), %0.f tiles: mfma_qk_p2c+stores %.0f | lds_sync %.0f | gather %.0f | "
                        "max+xchg %.0f | exp+sum %.0f | cvt+pv %.0f | c2p_next %.0f | total %.0f\n",
                nt, s[0] / nt, s[1] / nt, s[2] / nt, s[3] / nt, s[4] / nt, s[5] / nt, s[6] / nt,
                (s[0] + s[1] + s[2] + s[3] + s[4] + s[5] + s[6]) / nt);
    }
    return t / iters;
}

/* 1: this library was built with make DEV=1 (developer kernels, stamps and the GLC_* environment switches compiled in); 0: the product library. */
int glc_debug_is_developer_build(void) {
#ifdef GLC_DEVELOPER
    return 1;
#else
    return 0;
#endif
}

}  // extern "C"
