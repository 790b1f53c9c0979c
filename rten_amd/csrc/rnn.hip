// GRU and LSTM (src/ops/rnn.rs:138-328, 413-597): one recurrent layer, all directions, every value on the device.
//
// Arithmetic (one rounded f32 operation at a time, as the reference):
//     GRU   gates = x_t.W^T (+ Wb); hs = h.R^T (+ Rb); z, r = sigmoid(gates[z|r] + hs[z|r]); g = tanh(gates[h] + hs[h] * r);
//           h = (1 - z) * g + z * h
//     LSTM  gates = x_t.W^T (+ Wb); gates = 1 * gates + h.R^T (the addend enters the first depth block's store: cin + acc); (+ Rb);
//           i, o, f = sigmoid, g = tanh; c = f * c + i * g; h = o * tanh(c)   (vm::tanh here too -- the reference's f32::tanh is the host's libm)
// Products take the reference's depth-blocked order (k-ordered FMA chains from zero in blocks of 256, later blocks added to the earlier total); with ONE batch
// row and fewer than PREPACK_MIN_SEQ_LEN = 5 time steps the reference's operands are unpacked and its one-row kernels run instead: rten_hip_gemm_f32 makes
// that choice (rten_hip_set_gemv_order), so that case takes the composed path.
//
// Both paths hoist the input projection: x.W^T for all time steps of a direction is ONE launch of the f32 GEMM over [seq * batch, input] into a
// [seq, batch, G * hidden] workspace (each element's chain does not depend on which row it sits in: same bits as the per-step products).
//   composed  per step and direction: the f32 GEMM for h.R^T plus one gate kernel.  Any size.
//   fused     ONE launch for the whole layer: a workgroup owns 16 batch rows of one direction and walks all time steps itself (grid = batch tiles x
//             directions; no workgroup ever waits for another).  h lives in LDS (two buffers, one barrier per step), c and the lane's own h in registers.
//             h.R^T is v_mfma_f32_16x16x4_f32 chains: rows = 16 hidden units of one gate, columns = the 16 batch rows, depth = hidden in steps of 4 --
//             R re-laid once per call as [dir][gate][k / 4][unit][k % 4] (an A operand is 64 consecutive floats, streamed from L2).  Each of the 8 waves
//             owns up to 2 blocks of 16 hidden units with all their gates, so the gate arithmetic needs no exchange.  hidden <= RTEN_HIP_RNN_FUSED_MAX_HIDDEN
//             (256) is a register limit: 2 x G accumulator blocks plus the step's projection and both biases per lane; twice as many spill.
#include "internal.h"
#include "vecmath.h"

namespace {

typedef float rf4 __attribute__((ext_vector_type(4)));
extern __shared__ __attribute__((aligned(16))) float rnn_smem[];

constexpr int RNN_WAVES = 8; // waves per workgroup of the fused kernel

__device__ __forceinline__ bool rnn_reversed(int direction, int dir) { return (direction == 1 && dir == 0) || (direction == 2 && dir == 1); }

// state = src (or zeros)
__global__ __launch_bounds__(256) void rnn_init_state_kernel(float *__restrict__ dst, const float *__restrict__ src, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src ? src[i] : 0.0f;
}

// x[r][c] += bias[c]  (add_in_place of the input bias over every time step at once: LSTM, whose recurrent GEMM accumulates onto it)
__global__ __launch_bounds__(256) void rnn_add_row_bias_kernel(float *__restrict__ x, const float *__restrict__ bias, long long rows, int cols) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < rows * cols) x[i] = x[i] + bias[i % cols];
}

// R [dirs][G * H][H] -> [dirs][G][nsteps][JP][4]: element (unit j, depth k) at [k / 4][j][k % 4], zero where j >= H or k >= H
__global__ __launch_bounds__(256) void rnn_pack_r_kernel(const float *__restrict__ r, float *__restrict__ rp, int H, int G, int nsteps, int JP, long long total) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int q = (int)(e & 3);
    long long v = e >> 2;
    const int j = (int)(v % JP); v /= JP;
    const int st = (int)(v % nsteps); v /= nsteps; // v = dir * G + gate
    const int k = 4 * st + q;
    rp[e] = (j < H && k < H) ? r[(v * H + j) * H + k] : 0.0f;
}

struct GateArgs {
    const float *xp;  // [batch][GH]: x_t.W^T (GRU) / x_t.W^T + Wb + h.R^T (LSTM)
    const float *hs;  // GRU: [batch][GH] h.R^T
    const float *wb, *rb; // [GH] each or NULL
    float *h, *c;     // state [batch][H]
    float *y, *yh, *yc; // Y[t, dir] / final-state outputs (NULL: not written)
    int batch, H;
};

__global__ __launch_bounds__(256) void gru_gate_kernel(const GateArgs p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)p.batch * p.H) return;
    const int b = (int)(i / p.H), j = (int)(i - (long long)b * p.H);
    const long long row = (long long)b * 3 * p.H;
    float gz = p.xp[row + j], gr = p.xp[row + p.H + j], gh = p.xp[row + 2 * p.H + j];
    float hz = p.hs[row + j], hr = p.hs[row + p.H + j], hh = p.hs[row + 2 * p.H + j];
    if (p.wb) { gz = gz + p.wb[j]; gr = gr + p.wb[p.H + j]; gh = gh + p.wb[2 * p.H + j]; }
    if (p.rb) { hz = hz + p.rb[j]; hr = hr + p.rb[p.H + j]; hh = hh + p.rb[2 * p.H + j]; }
    const float z = vm::sigmoid(gz + hz), r = vm::sigmoid(gr + hr);
    hh = hh * r;
    const float g = vm::tanh(gh + hh);
    const float h = (1.0f - z) * g + z * p.h[i];
    p.h[i] = h;
    if (p.y) p.y[i] = h;
    if (p.yh) p.yh[i] = h;
}

__global__ __launch_bounds__(256) void lstm_gate_kernel(const GateArgs p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)p.batch * p.H) return;
    const int b = (int)(i / p.H), j = (int)(i - (long long)b * p.H);
    const long long row = (long long)b * 4 * p.H;
    float vi = p.xp[row + j], vo = p.xp[row + p.H + j], vf = p.xp[row + 2 * p.H + j], vc = p.xp[row + 3 * p.H + j];
    if (p.rb) { vi = vi + p.rb[j]; vo = vo + p.rb[p.H + j]; vf = vf + p.rb[2 * p.H + j]; vc = vc + p.rb[3 * p.H + j]; }
    const float ig = vm::sigmoid(vi), og = vm::sigmoid(vo), fg = vm::sigmoid(vf), cg = vm::tanh(vc);
    const float c = fg * p.c[i] + ig * cg;
    const float h = og * vm::tanh(c);
    p.c[i] = c;
    p.h[i] = h;
    if (p.y) p.y[i] = h;
    if (p.yh) p.yh[i] = h;
    if (p.yc) p.yc[i] = c;
}

struct FusedArgs {
    const float *xp;   // [dirs][seq][batch][GH]
    const float *rp;   // packed R
    const float *bias; // B [dirs][2 * GH] or NULL
    const float *h0, *c0; // [dirs][batch][H] or NULL
    float *y, *yh, *yc;   // NULL: not written
    int seq, batch, H, dirs, direction;
    int nsteps, JP, ld;
};

// One depth block of h.R^T for the NA active unit blocks of a wave: k-ordered chains, 4 MFMA steps' operands requested before the first multiply
template <int G, int NA>
__device__ __forceinline__ void rnn_chain(rf4 (&acc)[2][G], const float *__restrict__ rp, const float *hcur, int k0, int k1, int step_stride, int gate_stride) {
    int st = k0;
    for (; st + 4 <= k1; st += 4) {
        float hv[4], rv[4][NA][G];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            hv[u] = hcur[4 * (st + u)];
#pragma unroll
            for (int i = 0; i < NA; i++)
#pragma unroll
                for (int g = 0; g < G; g++) rv[u][i][g] = rp[g * gate_stride + (st + u) * step_stride + i * (16 * RNN_WAVES * 4)];
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int i = 0; i < NA; i++)
#pragma unroll
                for (int g = 0; g < G; g++) acc[i][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(rv[u][i][g], hv[u], acc[i][g], 0, 0, 0);
    }
    for (; st < k1; st++) {
        const float hv = hcur[4 * st];
#pragma unroll
        for (int i = 0; i < NA; i++)
#pragma unroll
            for (int g = 0; g < G; g++) acc[i][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(rp[g * gate_stride + st * step_stride + i * (16 * RNN_WAVES * 4)], hv, acc[i][g], 0, 0, 0);
    }
}

// A wave owns the unit blocks jt = wave and wave + 8 (hidden <= 256: one depth block, so a chain's end is the product)
template <bool LSTM>
__global__ __launch_bounds__(64 * RNN_WAVES) void rnn_fused_kernel(const FusedArgs p) {
    constexpr int G = LSTM ? 4 : 3, TPW = 2;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, quad = lane >> 4;
    const int dir = blockIdx.y, b0 = blockIdx.x * 16, b = b0 + l15;
    const bool bok = b < p.batch;
    const int H = p.H, GH = G * H, ld = p.ld;
    const bool rev = rnn_reversed(p.direction, dir);
    float *hbuf = rnn_smem; // [2][16][ld]
    for (int idx = t; idx < 16 * ld; idx += 64 * RNN_WAVES) {
        const int bb = idx / ld, k = idx - bb * ld;
        float v = 0.0f;
        if (p.h0 && b0 + bb < p.batch && k < H) v = p.h0[((long long)dir * p.batch + b0 + bb) * H + k];
        hbuf[idx] = v;
        hbuf[16 * ld + idx] = 0.0f;
    }
    // this lane's elements: batch row b, hidden units j = 16 * jt + 4 * quad + r of the wave's blocks jt = wave + 8 i
    const int nact = __builtin_amdgcn_readfirstlane(16 * wave >= p.JP ? 0 : 16 * (wave + RNN_WAVES) >= p.JP ? 1 : 2);
    float hreg[TPW][4], creg[TPW][4], rbv[TPW][G][4], wbv[TPW][G][4];
    const float *wb = p.bias ? p.bias + (long long)dir * 2 * GH : nullptr, *rb = wb ? wb + GH : nullptr;
#pragma unroll
    for (int i = 0; i < TPW; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = 16 * (wave + RNN_WAVES * i) + 4 * quad + r;
            const bool ok = bok && j < H;
            const long long si = ((long long)dir * p.batch + b) * H + j;
            hreg[i][r] = (ok && p.h0) ? p.h0[si] : 0.0f;
            creg[i][r] = (LSTM && ok && p.c0) ? p.c0[si] : 0.0f;
#pragma unroll
            for (int g = 0; g < G; g++) {
                rbv[i][g][r] = (rb && j < H) ? rb[g * H + j] : 0.0f;
                wbv[i][g][r] = (wb && j < H) ? wb[g * H + j] : 0.0f;
            }
        }
    const float *rpw = p.rp + ((long long)dir * G * p.nsteps * p.JP + 16 * wave + l15) * 4 + quad;
    const int step_stride = p.JP * 4, gate_stride = p.nsteps * step_stride;
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < p.seq; s++) {
        const int ts = rev ? p.seq - 1 - s : s;
        // the input projection of this step (+ Wb): independent of h, in flight during the product
        float xv[TPW][G][4];
        const float *xrow = p.xp + (((long long)dir * p.seq + ts) * p.batch + (bok ? b : 0)) * GH;
#pragma unroll
        for (int i = 0; i < TPW; i++)
#pragma unroll
            for (int g = 0; g < G; g++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int j = 16 * (wave + RNN_WAVES * i) + 4 * quad + r;
                    xv[i][g][r] = (bok && j < H) ? xrow[g * H + j] : 0.0f;
                }
        rf4 acc[TPW][G];
#pragma unroll
        for (int i = 0; i < TPW; i++)
#pragma unroll
            for (int g = 0; g < G; g++) acc[i][g] = rf4{0.f, 0.f, 0.f, 0.f};
        const float *hcur = hbuf + cur * 16 * ld + l15 * ld + quad;
        if (nact == 2) rnn_chain<G, 2>(acc, rpw, hcur, 0, p.nsteps, step_stride, gate_stride);
        else if (nact == 1) rnn_chain<G, 1>(acc, rpw, hcur, 0, p.nsteps, step_stride, gate_stride);
        float *hnext = hbuf + (cur ^ 1) * 16 * ld + l15 * ld;
#pragma unroll
        for (int i = 0; i < TPW; i++) {
            const int ju = 16 * (wave + RNN_WAVES * i);
            if (i >= nact) continue;
            float hn[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = ju + 4 * quad + r;
                float xg[G], v[G];
#pragma unroll
                for (int g = 0; g < G; g++) {
                    xg[g] = wb ? xv[i][g][r] + wbv[i][g][r] : xv[i][g][r];
                    v[g] = LSTM ? xg[g] + acc[i][g][r] : acc[i][g][r]; // LSTM: beta = 1, the addend enters the (only) depth block's store: cin + acc
                    if (rb) v[g] = v[g] + rbv[i][g][r];
                }
                float h;
                if (LSTM) {
                    const float ig = vm::sigmoid(v[0]), og = vm::sigmoid(v[1]), fg = vm::sigmoid(v[2]), cg = vm::tanh(v[G - 1]);
                    const float c = fg * creg[i][r] + ig * cg;
                    creg[i][r] = c;
                    h = og * vm::tanh(c);
                } else {
                    const float z = vm::sigmoid(xg[0] + v[0]), rr = vm::sigmoid(xg[1] + v[1]);
                    const float hh = v[2] * rr;
                    const float gg = vm::tanh(xg[2] + hh);
                    h = (1.0f - z) * gg + z * hreg[i][r];
                }
                h = (bok && j < H) ? h : 0.0f; // padding rows / units stay zero: they feed the next step's chains as exact zeros
                hreg[i][r] = h;
                hn[r] = h;
                if (p.y && bok && j < H) p.y[(((long long)ts * p.dirs + dir) * p.batch + b) * H + j] = h;
            }
            *reinterpret_cast<rf4 *>(hnext + ju + 4 * quad) = rf4{hn[0], hn[1], hn[2], hn[3]};
        }
        __syncthreads();
        cur ^= 1;
    }
#pragma unroll
    for (int i = 0; i < TPW; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = 16 * (wave + RNN_WAVES * i) + 4 * quad + r;
            if (!bok || j >= H) continue;
            const long long si = ((long long)dir * p.batch + b) * H + j;
            if (p.yh) p.yh[si] = hreg[i][r];
            if (LSTM && p.yc) p.yc[si] = creg[i][r];
        }
}

struct rten_hip_rnn_desc {
    int32_t seq, batch, input, hidden, direction;
    int64_t x_ss, x_bs;
};

inline size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }

template <bool LSTM>
int32_t launch_fused(rten_hip_ctx *ctx, const FusedArgs &a, size_t lds) {
    hipLaunchKernelGGL((rnn_fused_kernel<LSTM>), dim3((unsigned)((a.batch + 15) / 16), (unsigned)a.dirs), dim3(64 * RNN_WAVES), lds, ctx->stream, a);
    RTEN_LAUNCH_CHECK(ctx, "rnn_fused_kernel launch");
    return RTEN_HIP_OK;
}

int32_t rnn_run(rten_hip_ctx *ctx, const rten_hip_rnn_desc *d, bool lstm, const float *x, const float *w, const float *r, const float *b, const float *h0,
                const float *c0, float *y, float *yh, float *yc) {
    const char *op = lstm ? "lstm" : "gru";
    if (d->seq < 0 || d->batch < 0 || d->input < 0 || d->hidden < 0 || d->direction < 0 || d->direction > 2)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "%s: invalid geometry", op);
    const int G = lstm ? 4 : 3, dirs = d->direction == 2 ? 2 : 1;
    const int seq = d->seq, batch = d->batch, K = d->input, H = d->hidden;
    const long long GH = (long long)G * H, state_n = (long long)dirs * batch * H;
    if (GH > 0x7fffffffLL || (long long)seq * batch > 0x7fffffffLL || state_n > 0x7fffffffLL)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "%s: geometry too large", op);
    if (batch == 0 || H == 0) return RTEN_HIP_OK;
    const unsigned state_blocks = (unsigned)((state_n + 255) / 256);
    if (seq == 0) { // no step runs: the final states are the initial ones
        if (yh) hipLaunchKernelGGL(rnn_init_state_kernel, dim3(state_blocks), dim3(256), 0, ctx->stream, yh, h0, state_n);
        if (lstm && yc) hipLaunchKernelGGL(rnn_init_state_kernel, dim3(state_blocks), dim3(256), 0, ctx->stream, yc, c0, state_n);
        RTEN_LAUNCH_CHECK(ctx, "rnn_init_state_kernel launch");
        return RTEN_HIP_OK;
    }
    if (K == 0) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "%s: an input size of 0 is not supported", op);
    if (!x || !w || !r) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "%s: NULL operand", op);
    const long long x_bs = d->x_bs ? d->x_bs : K, x_ss = d->x_ss ? d->x_ss : (long long)batch * x_bs;

    // the reference's operands are unpacked below PREPACK_MIN_SEQ_LEN steps, and a one-row product of unpacked operands takes its gemv kernels
    const bool one_row = batch == 1 && seq < 5 && ctx->gemv_order != 0;
    const bool covered = H <= RTEN_HIP_RNN_FUSED_MAX_HIDDEN && !one_row;
    if (ctx->rnn_path == 2 && !covered)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "%s: the fused kernel does not cover this size (hidden <= %d, not the one-row gemv case)", op, RTEN_HIP_RNN_FUSED_MAX_HIDDEN);
    // automatic = composed until the fused kernel has measured faster at a size (docs/KERNELS.md 4.6: no timing exists yet); mode 2 selects it
    const bool fused = covered && ctx->rnn_path == 2;

    const int nsteps = (H + 3) / 4, JP = (H + 15) / 16 * 16;
    const size_t n_xp = align64((size_t)dirs * seq * batch * GH), n_state = align64((size_t)state_n), n_hs = align64((size_t)batch * GH);
    const size_t n_rp = align64((size_t)dirs * G * nsteps * JP * 4);
    const size_t floats = n_xp + (fused ? n_rp : 2 * n_state + n_hs);
    float *ws = (float *)rten_aux_scratch(ctx, floats * sizeof(float));
    if (!ws) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "%s: workspace allocation failed (or attempted during graph capture)", op);
    float *xp = ws;

    // ---- x.W^T for every time step of a direction: one launch
    for (int dir = 0; dir < dirs; dir++) {
        rten_hip_gemm_desc gd = {};
        gd.n = (int32_t)GH; gd.k = K;
        gd.a_cs = 1; gd.b_rs = 1; gd.b_cs = K; gd.ldc = GH;
        gd.alpha = 1.f; gd.beta = 0.f;
        const float *wd = w + (long long)dir * GH * K;
        float *xd = xp + (long long)dir * seq * batch * GH;
        int32_t rc;
        if (one_row) { // seq products of one row each, in the one-row order
            gd.m = 1; gd.a_rs = x_bs; gd.batch = seq; gd.a_bs = x_ss; gd.b_bs = 0; gd.c_bs = GH;
            rc = rten_hip_gemm_f32(ctx, &gd, x, wd, nullptr, xd);
        } else if (x_ss == (long long)batch * x_bs) {
            gd.m = seq * batch; gd.a_rs = x_bs; gd.batch = 1;
            rc = rten_gemm_f32_blocked(ctx, &gd, x, wd, nullptr, xd);
        } else {
            gd.m = batch; gd.a_rs = x_bs; gd.batch = seq; gd.a_bs = x_ss; gd.b_bs = 0; gd.c_bs = (long long)batch * GH;
            rc = rten_gemm_f32_blocked(ctx, &gd, x, wd, nullptr, xd);
        }
        if (rc) return rc;
    }

    if (fused) {
        float *rp = ws + n_xp;
        const long long total = (long long)dirs * G * nsteps * JP * 4;
        {
            ProfScope ps(ctx, "rnn_pack_r_kernel", 0.0, 8.0 * (double)total);
            hipLaunchKernelGGL(rnn_pack_r_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, r, rp, H, G, nsteps, JP, total);
            RTEN_LAUNCH_CHECK(ctx, "rnn_pack_r_kernel launch");
        }
        FusedArgs a;
        a.xp = xp; a.rp = rp; a.bias = b; a.h0 = h0; a.c0 = lstm ? c0 : nullptr; a.y = y; a.yh = yh; a.yc = lstm ? yc : nullptr;
        a.seq = seq; a.batch = batch; a.H = H; a.dirs = dirs; a.direction = d->direction;
        a.nsteps = nsteps; a.JP = JP; a.ld = (H + 63) / 64 * 64 + 4; // row pitch = 4 mod 64 banks: the 64 lanes of a B-operand read hit 64 banks
        const size_t lds = (size_t)2 * 16 * a.ld * sizeof(float);
        ProfScope ps(ctx, lstm ? "lstm_fused_kernel" : "gru_fused_kernel", 2.0 * seq * (double)dirs * batch * GH * H, 4.0 * ((double)seq * dirs * batch * (GH + H)));
        return lstm ? launch_fused<true>(ctx, a, lds) : launch_fused<false>(ctx, a, lds);
    }

    // ---- composed path
    float *hst = ws + n_xp, *cst = hst + n_state, *hs = cst + n_state;
    hipLaunchKernelGGL(rnn_init_state_kernel, dim3(state_blocks), dim3(256), 0, ctx->stream, hst, h0, state_n);
    if (lstm) hipLaunchKernelGGL(rnn_init_state_kernel, dim3(state_blocks), dim3(256), 0, ctx->stream, cst, c0, state_n);
    RTEN_LAUNCH_CHECK(ctx, "rnn_init_state_kernel launch");
    if (lstm && b) {
        for (int dir = 0; dir < dirs; dir++) {
            const long long rows = (long long)seq * batch;
            hipLaunchKernelGGL(rnn_add_row_bias_kernel, dim3((unsigned)((rows * GH + 255) / 256)), dim3(256), 0, ctx->stream, xp + (long long)dir * rows * GH,
                               b + (long long)dir * 2 * GH, rows, (int)GH);
        }
        RTEN_LAUNCH_CHECK(ctx, "rnn_add_row_bias_kernel launch");
    }
    const unsigned gate_blocks = (unsigned)(((long long)batch * H + 255) / 256);
    for (int dir = 0; dir < dirs; dir++) {
        const bool rev = (d->direction == 1 && dir == 0) || (d->direction == 2 && dir == 1);
        const float *rd = r + (long long)dir * GH * H;
        float *hd = hst + (long long)dir * batch * H, *cd = cst + (long long)dir * batch * H;
        for (int s = 0; s < seq; s++) {
            const int ts = rev ? seq - 1 - s : s;
            float *xt = xp + (((long long)dir * seq + ts) * batch) * GH;
            rten_hip_gemm_desc gd = {};
            gd.m = batch; gd.n = (int32_t)GH; gd.k = H;
            gd.a_rs = H; gd.a_cs = 1; gd.b_rs = 1; gd.b_cs = H; gd.ldc = GH; gd.batch = 1;
            gd.alpha = 1.f; gd.beta = lstm ? 1.f : 0.f;
            float *out = lstm ? xt : hs;
            const int32_t rc = one_row ? rten_hip_gemm_f32(ctx, &gd, hd, rd, nullptr, out) : rten_gemm_f32_blocked(ctx, &gd, hd, rd, nullptr, out);
            if (rc) return rc;
            GateArgs ga;
            ga.xp = xt; ga.hs = hs; ga.wb = b ? b + (long long)dir * 2 * GH : nullptr; ga.rb = ga.wb ? ga.wb + GH : nullptr;
            ga.h = hd; ga.c = cd; ga.batch = batch; ga.H = H;
            ga.y = y ? y + (((long long)ts * dirs + dir) * batch) * H : nullptr;
            const bool last = s == seq - 1;
            ga.yh = (last && yh) ? yh + (long long)dir * batch * H : nullptr;
            ga.yc = (last && lstm && yc) ? yc + (long long)dir * batch * H : nullptr;
            ProfScope ps(ctx, lstm ? "lstm_gate_kernel" : "gru_gate_kernel", 0.0, 4.0 * (double)batch * (GH + 3.0 * H));
            if (lstm) hipLaunchKernelGGL(lstm_gate_kernel, dim3(gate_blocks), dim3(256), 0, ctx->stream, ga);
            else hipLaunchKernelGGL(gru_gate_kernel, dim3(gate_blocks), dim3(256), 0, ctx->stream, ga);
            RTEN_LAUNCH_CHECK(ctx, "rnn gate kernel launch");
        }
    }
    return RTEN_HIP_OK;
}

} // namespace

RTEN_EXPORT int32_t rten_hip_set_rnn_path(rten_hip_ctx *ctx, int32_t mode) {
    RTEN_CHECK_CTX(ctx);
    if (mode < 0 || mode > 2) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "set_rnn_path: mode must be 0, 1 or 2");
    ctx->rnn_path = mode;
    return RTEN_HIP_OK;
}

RTEN_EXPORT int32_t rten_hip_gru_f32(rten_hip_ctx *ctx, int32_t seq, int32_t batch, int32_t input, int32_t hidden, int32_t direction,
                                     int32_t linear_before_reset, int64_t x_ss, int64_t x_bs, const float *x, const float *w, const float *r, const float *b,
                                     const float *initial_h, float *y, float *y_h) {
    RTEN_CHECK_CTX(ctx);
    const rten_hip_rnn_desc desc = {seq, batch, input, hidden, direction, x_ss, x_bs}, *d = &desc;
    if (!linear_before_reset) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "`linear_before_reset=0` is not supported"); // rnn.rs:153-158
    return rnn_run(ctx, d, false, x, w, r, b, initial_h, nullptr, y, y_h, nullptr);
}

RTEN_EXPORT int32_t rten_hip_lstm_f32(rten_hip_ctx *ctx, int32_t seq, int32_t batch, int32_t input, int32_t hidden, int32_t direction, int64_t x_ss,
                                      int64_t x_bs, const float *x, const float *w, const float *r, const float *b, const float *initial_h,
                                      const float *initial_c, float *y, float *y_h, float *y_c) {
    RTEN_CHECK_CTX(ctx);
    const rten_hip_rnn_desc desc = {seq, batch, input, hidden, direction, x_ss, x_bs}, *d = &desc;
    return rnn_run(ctx, d, true, x, w, r, b, initial_h, initial_c, y, y_h, y_c);
}
