// Staging for the fast int8 path (int8_fast.h: the layouts): the kernels that bring weights, activations and f32 tensors into the operands igemm_i8_fast_kernel
// reads, their launchers, and the entry points that only stage -- prepacking at load, the staged forms of DynamicQuantizeLinear, the statistics blocks.
#include "int8_fast.h"
#include "quantize.h"
#include "vecmath.h"

namespace {

__device__ __forceinline__ int zp_signed(const uint8_t *zp, int idx, int is_signed) {
    if (!zp) return is_signed ? 0 : -128;
    return is_signed ? (int)(int8_t)zp[idx] : (int)zp[idx] - 128;
}

// rows of a strided u8/i8 matrix -> chunk-major signed operand [Kp/16][rows][16 B] (+ row sums).  With khw > 1 the
// source k index is (c, tap) (OIHW weights) and the destination k index is (tap, c) with channels padded to Cp.
// `pk_nch` > 0: the few-channel PACKED destination order (conv_geom, round 6): chunk (ky, j) holds kernel columns j * pk_cpc .. + pk_cpc - 1 of row ky, byte
// col * C + channel; columns past the kernel's width and the bytes past pk_cpc * C are zero weights.
__global__ __launch_bounds__(256) void i8_pack_rows_kernel(const uint8_t *__restrict__ src, long long row_stride, long long k_stride, int K,
                                                          int C, int khw, int Cp, int Kp, int rows, unsigned flip, uint8_t *__restrict__ dst,
                                                          int *__restrict__ sums, int pk_nch = 0, int pk_cpc = 0, int pk_kw = 0) {
    const int r = blockIdx.x;
    const uint8_t *s = src + (long long)r * row_stride;
    int sum = 0;
    for (int kq = threadIdx.x * 4; kq < Kp; kq += 1024) {
        unsigned w = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int kd = kq + b;
            int tap = kd / Cp, c = kd - tap * Cp;
            bool ok = tap < khw && c < C;
            if (pk_nch > 0) { // (Cp == 16 here; `khw` = kernel rows x kernel columns of the REAL kernel)
                const int vt = kd >> 4, slot = kd & 15, ky = vt / pk_nch, j = vt - ky * pk_nch, col = slot / C, kx = j * pk_cpc + col;
                c = slot - col * C;
                ok = ky * pk_kw < khw && col < pk_cpc && kx < pk_kw;
                tap = ky * pk_kw + kx;
            }
            const int ks = c * khw + tap;
            const unsigned v = ok ? ((unsigned)s[(long long)(ks < K ? ks : 0) * k_stride] ^ flip) & 0xffu : 0u;
            w |= v << (8 * b);
        }
        *reinterpret_cast<unsigned *>(dst + ((long long)(kq >> 4) * rows + r) * 16 + (kq & 15)) = w;
        sum = __builtin_amdgcn_sdot4((int)w, 0x01010101, sum, false);
    }
    __shared__ int red[4];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) sums[r] = red[0] + red[1] + red[2] + red[3];
}

// Transposing variant of the row packer for operands whose rows are NOT k-contiguous (e.g. MatMulInteger weights
// [K][N]: row n walks k with stride N).  64 x 64 byte tiles through LDS: coalesced reads along the source's
// contiguous axis, 4-byte writes along k.  Row sums via atomics into a zeroed array.
__global__ __launch_bounds__(256) void i8_pack_rows_t_kernel(const uint8_t *__restrict__ src, long long row_stride, long long k_stride, int rows,
                                                            int K, int Kp, unsigned flip, uint8_t *__restrict__ dst, int *__restrict__ sums) {
    __shared__ uint8_t tile[64][64 + 4];
    const int t = threadIdx.x;
    const int r0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
    // read: consecutive threads walk rows (the source's contiguous axis when row_stride == 1)
#pragma unroll
    for (int pass = 0; pass < 16; pass++) {
        const int rl = t & 63, kl = pass * 4 + (t >> 6);
        const int r = r0 + rl, k = k0 + kl;
        unsigned v = 0;
        if (r < rows && k < K) v = ((unsigned)src[(long long)r * row_stride + (long long)k * k_stride] ^ flip) & 0xffu;
        tile[rl][kl] = (uint8_t)v;
    }
    __syncthreads();
    // write: thread -> (row, 16-byte group), consecutive lanes on consecutive rows of one chunk plane; k0 + 64 <= Kp
    // always (Kp is a multiple of 64)
    const int rl = t & 63, g = t >> 6;
    const int r = r0 + rl;
    int sum = 0;
    if (r < rows) {
        unsigned w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            w[q] = (unsigned)tile[rl][g * 16 + q * 4] | ((unsigned)tile[rl][g * 16 + q * 4 + 1] << 8) | ((unsigned)tile[rl][g * 16 + q * 4 + 2] << 16) |
                   ((unsigned)tile[rl][g * 16 + q * 4 + 3] << 24);
            sum = __builtin_amdgcn_sdot4((int)w[q], 0x01010101, sum, false);
        }
        *reinterpret_cast<uint4 *>(dst + ((long long)(k0 / 16 + g) * rows + r) * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (r < rows) atomicAdd(&sums[r], sum);
}

// Staging of conv activations: NCHW -> padded channel-blocked signed bytes [N][Cp/16][Hp][Wp][16 B]; border = pad
// value of the selected mode, padded channels 0.  A workgroup takes 256 consecutive SOURCE pixels of one image x one
// 16-channel block: a thread loads 4 consecutive pixels (one 16-byte load when the plane size allows) of 4 consecutive
// channels, packs the 4 channel bytes of each pixel into a dword and parks them in LDS ([channel quad][pixel], one
// conflict-free ds_write_b128); the workgroup then writes the run of PADDED positions that its pixels span -- border
// pieces included -- as consecutive 16-byte pieces (1 KiB per wave instruction).  `prep()` runs AFTER the loads are in
// flight (so e.g. the statistics fold of the fused quantizer hides behind them) and returns the mapping: `.fill` =
// signed-domain border byte, `.byte(v)` = source element -> signed-domain byte.
template <typename T> struct Vec4;
template <> struct Vec4<float> { typedef float4 type; };
template <> struct Vec4<uint8_t> { typedef uchar4 type; };

template <typename T, bool VEC, typename Prep>
__device__ __forceinline__ void stage_blocked_tile(const T *__restrict__ x, uint8_t *__restrict__ xp, int C, int H, int W, int Hp, int Wp, int Cp, int pt, int pl,
                                                   Prep prep) {
    __shared__ __attribute__((aligned(16))) unsigned tile[4][256];
    const int t = threadIdx.x;
    const int HW = H * W, npix = Hp * Wp;
    const int p0 = blockIdx.x * 256, n = blockIdx.y, cb = blockIdx.z;
    const int px = (t & 63) * 4, cq = (t >> 6) * 4;
    T raw[4][4]; // [channel][pixel]
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int c = cb * 16 + cq + j;
        const long long base = ((long long)n * C + (c < C ? c : 0)) * HW + p0 + px;
        if constexpr (VEC) { // HW % 4 == 0: the 4 pixels are all inside or all outside, and the address is 4-element aligned
            const typename Vec4<T>::type v = *reinterpret_cast<const typename Vec4<T>::type *>(x + ((c < C && p0 + px < HW) ? base : 0));
            raw[j][0] = v.x; raw[j][1] = v.y; raw[j][2] = v.z; raw[j][3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) raw[j][i] = x[(c < C && p0 + px + i < HW) ? base + i : 0];
        }
    }
    const auto map = prep();
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        w[i] = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned v = (cb * 16 + cq + j < C) ? map.byte(raw[j][i]) & 0xffu : 0u;
            w[i] |= v << (8 * j);
        }
    }
    *reinterpret_cast<uint4 *>(&tile[t >> 6][px]) = make_uint4(w[0], w[1], w[2], w[3]);
    __syncthreads();
    // border piece of this channel block: pad byte on real channels, 0 on the padding channels
    unsigned fw[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        fw[q] = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) fw[q] |= (cb * 16 + q * 4 + j < C ? map.fill : 0u) << (8 * j);
    }
    auto padded = [&](int sp) { const int y = sp / W; return (y + pt) * Wp + (sp - y * W) + pl; };
    const int s_end = p0 + 256 < HW ? p0 + 256 : HW;
    const int begin = p0 == 0 ? 0 : padded(p0);
    const int end = s_end == HW ? npix : padded(s_end);
    uint8_t *dst = xp + ((long long)n * (Cp / 16) + cb) * npix * 16;
    for (int pp = begin + t; pp < end; pp += 256) {
        const int yp = pp / Wp, xq = pp - yp * Wp;
        const int y = yp - pt, xs = xq - pl;
        uint4 v = make_uint4(fw[0], fw[1], fw[2], fw[3]);
        if ((unsigned)y < (unsigned)H && (unsigned)xs < (unsigned)W) {
            const int sl = y * W + xs - p0; // in [0, 256): the padded run [begin, end) covers exactly this workgroup's pixels
            v = make_uint4(tile[0][sl], tile[1][sl], tile[2][sl], tile[3][sl]);
        }
        *reinterpret_cast<uint4 *>(dst + (long long)pp * 16) = v;
    }
}

// Few-channel PACKED staging (round 6; conv_geom): a convolution with C <= 4 input channels (the 7x7 / stride 2 stem of ResNet-50: C = 3) staged as a 16-channel
// block moves 16 bytes per pixel for 3 of data and multiplies 13 zeros per tap (K = 49 x 16 = 784 for 147 real terms).  Here a 16-byte chunk holds `cpc` = 16 / C
// horizontally adjacent kernel COLUMNS x C channels of one kernel row, and every OUTPUT column gets its own `nch` = ceil(KW / cpc) chunks per padded input row
// (columns ox * stride - pad + j * cpc + col): image [N][Hp][OW * nch][16 B], which the unchanged kernel walks as a convolution with 16 channels, KW = nch and
// stride nch over "virtual columns" -- K = KH x nch x 16 (224 for the stem).  A thread writes one chunk: all its (clamped) loads first, then `prep()`.
template <typename T, int C, int NCH, typename Prep>
__device__ __forceinline__ void stage_packed_chunks(const T *__restrict__ x, uint8_t *__restrict__ xp, int H, int W, int Hp, int OW, int KW, int sx, int dx, int pt, int pl,
                                                    Prep prep) {
    // a thread owns one OUTPUT column of one padded input row: the NCH chunks of that column (32 consecutive bytes for the stem); grid = (OW / 128, Hp / 2, N).  The
    // channel count and the chunk count are compile-time, so the slot -> (kernel column, channel) map costs nothing; every load is issued (clamped) before prep().
    constexpr int CPC = 16 / C;
    // (256 threads = two padded rows x 128 output columns: prep()'s statistics fold is written for 256-thread workgroups)
    const int ox = blockIdx.x * 128 + (threadIdx.x & 127), ypr = blockIdx.y * 2 + (threadIdx.x >> 7), n = blockIdx.z;
    const int oxc = ox < OW ? ox : OW - 1, yp = ypr < Hp ? ypr : Hp - 1;
    const int y = yp - pt, x0 = oxc * sx - pl; // kernel column kx reads input column ox * stride - pad + kx * dilation
    const bool row_in = (unsigned)y < (unsigned)H;
    const long long plane = (long long)H * W;
    const T *row = x + (long long)n * C * plane + (long long)(row_in ? y : 0) * W;
    T raw[NCH * CPC][C];
#pragma unroll
    for (int kx = 0; kx < NCH * CPC; kx++) {
        const int xx = x0 + kx * dx;
        const bool in = kx < KW && row_in && (unsigned)xx < (unsigned)W;
#pragma unroll
        for (int ch = 0; ch < C; ch++) raw[kx][ch] = row[in ? ch * plane + xx : 0];
    }
    const auto map = prep();
#pragma unroll
    for (int j = 0; j < NCH; j++) {
        unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int col = 0; col < CPC; col++) {
            const int kx = j * CPC + col, xx = x0 + kx * dx;
            const bool real = kx < KW;                                        // a kernel column (else: a zero weight multiplies the byte, and the byte is 0)
            const bool in = real && row_in && (unsigned)xx < (unsigned)W;
#pragma unroll
            for (int ch = 0; ch < C; ch++) {
                constexpr int dummy = 0; (void)dummy;
                const int slot = col * C + ch;
                const unsigned v = in ? map.byte(raw[kx][ch]) & 0xffu : (real ? map.fill : 0u);
                w[slot >> 2] |= v << (8 * (slot & 3));
            }
        }
        if (ox < OW && ypr < Hp) *reinterpret_cast<uint4 *>(xp + ((((long long)n * Hp + yp) * OW + ox) * NCH + j) * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// Small feature maps (fewer than 128 pixels per plane, e.g. 7x7): 64 consecutive PADDED positions x 64 channels per
// workgroup, one pixel per lane, so the lanes stay busy where the 256-pixel tile above would idle.
template <typename T, typename Prep>
__device__ __forceinline__ void stage_blocked_tile_small(const T *__restrict__ x, uint8_t *__restrict__ xp, int C, int H, int W, int Hp, int Wp, int Cp, int pt, int pl,
                                                Prep prep) {
    __shared__ uint8_t tile[64][64 + 16];
    const int t = threadIdx.x;
    const int pp0 = blockIdx.x * 64, n = blockIdx.y;
    const int npix = Hp * Wp;
    const int pl_ = t & 63, pp = pp0 + pl_;
    const int yp = pp / Wp, xq = pp - yp * Wp;
    const int y = yp - pt, xs = xq - pl;
    const bool in = pp < npix && (unsigned)y < (unsigned)H && (unsigned)xs < (unsigned)W;
    const long long src0 = ((long long)n * C * H + (in ? y : 0)) * W + (in ? xs : 0); // + c * H * W
    const int c0 = blockIdx.z * 64; // one 64-channel slab per workgroup: small feature maps still give thousands of workgroups
    // thread -> (pixel, 4 consecutive channels) per pass.  All 16 loads are issued first (clamped address, no branch
    // around a load), then converted and packed: one dword per pass into the LDS tile.
    T raw[16];
#pragma unroll
    for (int pass = 0; pass < 4; pass++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int c = c0 + pass * 16 + (t >> 6) * 4 + b;
            raw[pass * 4 + b] = x[(in && c < C) ? src0 + (long long)c * H * W : 0];
        }
    const auto map = prep();
    const unsigned fill = map.fill;
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
        const int cl = pass * 16 + (t >> 6) * 4;
        unsigned w = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int c = c0 + cl + b;
            const unsigned v = (in && c < C) ? map.byte(raw[pass * 4 + b]) & 0xffu : (c < C ? fill : 0u);
            w |= v << (8 * b);
        }
        *reinterpret_cast<unsigned *>(&tile[pl_][cl]) = w;
    }
    __syncthreads();
    const int px = t & 63, ch = t >> 6;
    if (pp0 + px < npix && c0 + ch * 16 < Cp)
        *reinterpret_cast<uint4 *>(xp + (((long long)n * (Cp / 16) + (c0 / 16 + ch)) * npix + pp0 + px) * 16) = *reinterpret_cast<const uint4 *>(&tile[px][ch * 16]);
}

struct FlipMap {
    unsigned fill, flip;
    __device__ __forceinline__ unsigned byte(uint8_t b) const { return ((unsigned)b ^ flip) & 0xffu; }
};
struct QuantMap {
    unsigned fill;
    float inv_scale;
    int zp;
    __device__ __forceinline__ unsigned byte(float f) const { return dql::quant_u8(f, inv_scale, zp) ^ 0x80u; }
};

template <int KIND> // 0 = small maps, 1 = 256-pixel tiles with scalar loads, 2 = with 4-pixel vector loads
__global__ __launch_bounds__(256) void i8_nhwc_pad_kernel(const uint8_t *__restrict__ x, uint8_t *__restrict__ xp, int C, int H, int W, int Hp,
                                                         int Wp, int Cp, int pt, int pl, unsigned flip, const uint8_t *__restrict__ x_zp,
                                                         int x_signed, int pad_mode) {
    auto prep = [&]() {
        int pad_s = 0;
        if (pad_mode == RTEN_HIP_PAD_ZERO_POINT) pad_s = zp_signed(x_zp, 0, x_signed);
        else if (pad_mode == RTEN_HIP_PAD_RAW0_U8) pad_s = -128;
        return FlipMap{(unsigned)pad_s & 0xffu, flip};
    };
    if constexpr (KIND == 0) stage_blocked_tile_small(x, xp, C, H, W, Hp, Wp, Cp, pt, pl, prep);
    else stage_blocked_tile<uint8_t, KIND == 2>(x, xp, C, H, W, Hp, Wp, Cp, pt, pl, prep);
}

// DynamicQuantizeLinear's quantize sweep fused with the staging above: f32 NCHW -> u8 codes (bit-identical to
// quantize.hip: same scale / zero-point algebra, same to_int_round + saturate) written as padded channel-blocked
// signed bytes.  The min/max fold runs while the tile's loads are in flight.
// the scalar Mul(x_scale, w_scale) nodes that follow a DynamicQuantizeLinear in ort-quantized graphs (one per convolution that reads the
// quantized tensor: a stage's shortcut and first 1x1 convolution share one): product[i] = scale * mul_by[i][0]
constexpr int kMaxProducts = 4;
struct ScaleProducts {
    int count;
    const float *mul_by[kMaxProducts];
    float *product[kMaxProducts];
};

template <int C, int NCH>
__global__ __launch_bounds__(256) void i8_pad_packed_kernel(const uint8_t *__restrict__ x, uint8_t *__restrict__ xp, int H, int W, int Hp, int OW, int KW, int sx, int dx, int pt,
                                                           int pl, unsigned flip, const uint8_t *__restrict__ x_zp, int x_signed, int pad_mode) {
    auto prep = [&]() {
        int pad_s = 0;
        if (pad_mode == RTEN_HIP_PAD_ZERO_POINT) pad_s = zp_signed(x_zp, 0, x_signed);
        else if (pad_mode == RTEN_HIP_PAD_RAW0_U8) pad_s = -128;
        return FlipMap{(unsigned)pad_s & 0xffu, flip};
    };
    stage_packed_chunks<uint8_t, C, NCH>(x, xp, H, W, Hp, OW, KW, sx, dx, pt, pl, prep);
}

template <int KIND>
__global__ __launch_bounds__(256) void i8_quantize_stage_kernel(const float *__restrict__ x, const float *__restrict__ ws, int nparts, uint8_t *__restrict__ xp,
                                                               int C, int H, int W, int Hp, int Wp, int Cp, int pt, int pl, int pad_mode,
                                                               float *scale_out, uint8_t *zp_out, const ScaleProducts sp) {
    // explicit arguments: 0x58 bytes + ScaleProducts = 160 bytes, three lines (the tail of them is first touched AFTER the tile has arrived: on the critical path)
    kernarg_prefetch<0x58 + (int)sizeof(ScaleProducts)>();
    auto prep = [&]() {
        float x_min, x_max;
        if (nparts < 0) dql::block_minmax_slots(reinterpret_cast<const unsigned *>(ws), x_min, x_max); // producer-accumulated statistics
        else dql::block_minmax(ws, nparts, x_min, x_max);
        const dql::QParams q = dql::dql_params(x_min, x_max);
        if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
            *scale_out = q.scale;
            *zp_out = (uint8_t)q.zp;
#pragma unroll
            for (int i = 0; i < kMaxProducts; i++)
                if (i < sp.count) *sp.product[i] = q.scale * sp.mul_by[i][0];
        }
        int pad_s = 0; // signed-domain padding value
        if (pad_mode == RTEN_HIP_PAD_ZERO_POINT) pad_s = q.zp - 128;
        else if (pad_mode == RTEN_HIP_PAD_RAW0_U8) pad_s = -128;
        return QuantMap{(unsigned)pad_s & 0xffu, q.inv_scale, q.zp};
    };
    if constexpr (KIND == 0) stage_blocked_tile_small(x, xp, C, H, W, Hp, Wp, Cp, pt, pl, prep);
    else stage_blocked_tile<float, KIND == 2>(x, xp, C, H, W, Hp, Wp, Cp, pt, pl, prep);
}

// ... and DynamicQuantizeLinear's quantize sweep into the few-channel packed image (same prep as i8_quantize_stage_kernel: same codes)
template <int C, int NCH>
__global__ __launch_bounds__(256) void i8_quantize_packed_kernel(const float *__restrict__ x, const float *__restrict__ ws, int nparts, uint8_t *__restrict__ xp, int H, int W, int Hp,
                                                                int OW, int KW, int sx, int dx, int pt, int pl, int pad_mode, float *scale_out, uint8_t *zp_out,
                                                                const ScaleProducts sp) {
    auto prep = [&]() {
        float x_min, x_max;
        if (nparts < 0) dql::block_minmax_slots(reinterpret_cast<const unsigned *>(ws), x_min, x_max);
        else dql::block_minmax(ws, nparts, x_min, x_max);
        const dql::QParams q = dql::dql_params(x_min, x_max);
        if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
            *scale_out = q.scale;
            *zp_out = (uint8_t)q.zp;
#pragma unroll
            for (int i = 0; i < kMaxProducts; i++)
                if (i < sp.count) *sp.product[i] = q.scale * sp.mul_by[i][0];
        }
        int pad_s = 0;
        if (pad_mode == RTEN_HIP_PAD_ZERO_POINT) pad_s = q.zp - 128;
        else if (pad_mode == RTEN_HIP_PAD_RAW0_U8) pad_s = -128;
        return QuantMap{(unsigned)pad_s & 0xffu, q.inv_scale, q.zp};
    };
    stage_packed_chunks<float, C, NCH>(x, xp, H, W, Hp, OW, KW, sx, dx, pt, pl, prep);
}

__global__ void stats_reset_kernel(unsigned *stats, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per slot word
    if (i < count * 2 * dql::kStatSlots) stats[i] = (i % (2 * dql::kStatSlots)) < dql::kStatSlots ? 0xffffffffu : 0u; // minima | maxima
}

// Launchers: the grid of each staging form and the choice between its kernels, once for the u8 and the f32 source.  The packed form: channel count x chunks
// per output column, the instantiations conv_geom admits; 128 output columns x two padded rows per workgroup
#define RTEN_PACKED_DISPATCH(KERNEL, d, g, ...)                                                                                          \
    do {                                                                                                                                 \
        const dim3 grid((unsigned)(((d)->out_w + 127) / 128), (unsigned)(((g).Hp + 1) / 2), (unsigned)(d)->n);                            \
        switch ((d)->c * 4 + (g).nch) {                                                                                                  \
        case 1 * 4 + 1: hipLaunchKernelGGL((KERNEL<1, 1>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__); break;                         \
        case 1 * 4 + 2: hipLaunchKernelGGL((KERNEL<1, 2>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__); break;                         \
        case 2 * 4 + 1: hipLaunchKernelGGL((KERNEL<2, 1>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__); break;                         \
        case 2 * 4 + 2: hipLaunchKernelGGL((KERNEL<2, 2>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__); break;                         \
        case 3 * 4 + 1: hipLaunchKernelGGL((KERNEL<3, 1>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__); break;                         \
        case 3 * 4 + 2: hipLaunchKernelGGL((KERNEL<3, 2>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__); break;                         \
        case 4 * 4 + 1: hipLaunchKernelGGL((KERNEL<4, 1>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__); break;                         \
        default: hipLaunchKernelGGL((KERNEL<4, 2>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__); break;                                \
        }                                                                                                                                \
    } while (0)

// The channel-blocked form of a source image `x` of element size ELEM: small maps take KIND 0 (64 padded positions x 64 channels per workgroup), the others
// 256 source pixels x 16 channels per workgroup, with 4-pixel vector loads (KIND 2) where the plane size and the address allow them
#define RTEN_BLOCKED_DISPATCH(KERNEL, d, g, x, ELEM, ...)                                                                                \
    do {                                                                                                                                 \
        const dim3 grid((unsigned)(((d)->h * (d)->w + 255) / 256), (unsigned)(d)->n, (unsigned)((g).Cp / 16));                            \
        const dim3 grid_small((unsigned)(((g).Hp * (g).Wp + 63) / 64), (unsigned)(d)->n, (unsigned)(((g).Cp + 63) / 64));                 \
        const bool vec = ((d)->h * (d)->w) % 4 == 0 && ((uintptr_t)(x) & (4 * (ELEM) - 1)) == 0;                                          \
        if ((d)->h * (d)->w < 128) hipLaunchKernelGGL(KERNEL<0>, grid_small, dim3(256), 0, ctx->stream, __VA_ARGS__);                    \
        else if (vec) hipLaunchKernelGGL(KERNEL<2>, grid, dim3(256), 0, ctx->stream, __VA_ARGS__);                                       \
        else hipLaunchKernelGGL(KERNEL<1>, grid, dim3(256), 0, ctx->stream, __VA_ARGS__);                                                \
    } while (0)

// The three staged forms of DynamicQuantizeLinear behind their argument checks: quantize and stage an f32 image.  With `stats` the producer's statistics block
// gives min / max (the kernels' `nparts` < 0); without it a min / max sweep of `x` runs first and leaves per-workgroup partials.
int32_t quantize_staged(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const float *x, const void *stats, void *staged, float *scale, uint8_t *zero_point,
                        const ScaleProducts &sp) {
    const ConvGeom g = rten_i8_conv_geom(di);
    if (!g.ok || di->x_signed) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "quantize_staged: geometry not covered by the staged kernel (staged_bytes == 0)");
    const rten_hip_conv2d_desc *d = &di->conv;
    const int64_t n = (int64_t)d->n * d->c * d->h * d->w;
    const int pad_mode = rten_effective_pad_mode(di);
    ProfScope ps(ctx, stats ? "dynamic_quantize_linear_staged_stats" : "dynamic_quantize_linear_staged", 0.0, (stats ? 4.0 : 8.0) * n + (double)g.img);
    int nparts = -1;
    const float *ws = stats ? (const float *)stats : rten_dql_minmax(ctx, n, x, &nparts);
    if (!ws) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "dql: scratch allocation failed");
    if (g.packed)
        RTEN_PACKED_DISPATCH(i8_quantize_packed_kernel, d, g, x, ws, nparts, (uint8_t *)staged, d->h, d->w, g.Hp, d->out_w, d->kw, d->stride_w, d->dil_w, d->pads[0],
                             d->pads[1], pad_mode, scale, zero_point, sp);
    else
        RTEN_BLOCKED_DISPATCH(i8_quantize_stage_kernel, d, g, x, sizeof(float), x, ws, nparts, (uint8_t *)staged, d->c, d->h, d->w, g.Hp, g.Wp, g.Cp, d->pads[0],
                              d->pads[1], pad_mode, scale, zero_point, sp);
    RTEN_LAUNCH_CHECK(ctx, "i8_quantize_stage_kernel launch");
    return RTEN_HIP_OK;
}

ScaleProducts one_product(const float *mul_by, float *product) {
    ScaleProducts sp = {};
    if (mul_by) { sp.count = 1; sp.mul_by[0] = mul_by; sp.product[0] = product; }
    return sp;
}

} // namespace

ConvGeom rten_i8_conv_geom(const rten_hip_conv2d_int8_desc *di) {
    const rten_hip_conv2d_desc *d = &di->conv;
    ConvGeom g = {};
    g.Cp = (d->c + 15) / 16 * 16;
    g.Hp = d->h + d->pads[0] + d->pads[2];
    g.Wp = d->w + d->pads[1] + d->pads[3];
    g.taps = d->kh * d->kw;
    g.Kreal = d->c * g.taps;
    g.P = d->out_h * d->out_w;
    g.sx = d->stride_w; g.kw = d->kw; g.dx = d->dil_w;
    static const bool no_pack = getenv("RTEN_I8_NO_PACK") != nullptr; // (A/B switch: the 16-channel-block form for every geometry)
    if (!no_pack && d->groups == 1 && d->c >= 1 && d->c <= 4 && d->kw >= 2 && d->out_w > 0) {
        g.cpc = 16 / d->c;
        g.nch = (d->kw + g.cpc - 1) / g.cpc;
        if (g.nch < d->kw && g.nch <= 2) { // fewer chunks per kernel row than taps: the smaller product (one or two chunks per output column are instantiated)
            g.packed = true;
            g.Cp = 16;
            g.Wp = d->out_w * g.nch;
            g.taps = d->kh * g.nch;
            g.sx = g.nch; g.kw = g.nch; g.dx = 1;
        }
    }
    g.Kp = (g.taps * g.Cp + KT - 1) / KT * KT;
    g.img = (size_t)d->n * g.Hp * g.Wp * g.Cp;
    g.ok = d->groups == 1 && d->c > 0 && d->o > 0 && g.Kp <= (1 << 18) && // (the kernel's chunk -> offset table lives in LDS)
           // the chunk walk addresses taps on the padded image: the window must fit (true for valid conv geometry)
           (d->out_h - 1) * d->stride_h + (d->kh - 1) * d->dil_h < g.Hp && (d->out_w - 1) * g.sx + (g.kw - 1) * g.dx < g.Wp &&
           g.img < (1ull << 31) && (size_t)d->o * g.Kp < (1ull << 31) && (long long)d->n * d->o * g.P < (1ll << 29);
    return g;
}

void rten_i8_pack_rows(rten_hip_ctx *ctx, const void *src, long long row_stride, long long k_stride, int rows, int k, int Kp, unsigned flip, char *dst, char *sums) {
    if (k_stride == 1) {
        hipLaunchKernelGGL(i8_pack_rows_kernel, dim3((unsigned)rows), dim3(256), 0, ctx->stream, (const uint8_t *)src, row_stride, k_stride, k, k, 1, Kp, Kp, rows, flip,
                           (uint8_t *)dst, (int *)sums);
    } else {
        hipMemsetAsync(sums, 0, (size_t)rows * 4, ctx->stream);
        hipLaunchKernelGGL(i8_pack_rows_t_kernel, dim3((unsigned)((rows + 63) / 64), (unsigned)(Kp / 64)), dim3(256), 0, ctx->stream, (const uint8_t *)src, row_stride, k_stride,
                           rows, k, Kp, flip, (uint8_t *)dst, (int *)sums);
    }
}

void rten_i8_pack_conv_weights(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const ConvGeom &g, const void *w, void *dst, void *sums) {
    const rten_hip_conv2d_desc *d = &di->conv;
    hipLaunchKernelGGL(i8_pack_rows_kernel, dim3((unsigned)d->o), dim3(256), 0, ctx->stream, (const uint8_t *)w, (long long)g.Kreal, 1ll, g.Kreal, d->c, d->kh * d->kw,
                       g.Cp, g.Kp, d->o, di->w_signed ? 0u : 0x80u, (uint8_t *)dst, (int *)sums, g.packed ? g.nch : 0, g.cpc, d->kw);
}

void rten_i8_stage_image(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const ConvGeom &g, const void *x, const void *x_zp, void *staged) {
    const rten_hip_conv2d_desc *d = &di->conv;
    const unsigned flip = di->x_signed ? 0u : 0x80u;
    if (g.packed)
        RTEN_PACKED_DISPATCH(i8_pad_packed_kernel, d, g, (const uint8_t *)x, (uint8_t *)staged, d->h, d->w, g.Hp, d->out_w, d->kw, d->stride_w, d->dil_w, d->pads[0],
                             d->pads[1], flip, (const uint8_t *)x_zp, di->x_signed, rten_effective_pad_mode(di));
    else
        RTEN_BLOCKED_DISPATCH(i8_nhwc_pad_kernel, d, g, x, sizeof(uint8_t), (const uint8_t *)x, (uint8_t *)staged, d->c, d->h, d->w, g.Hp, g.Wp, g.Cp, d->pads[0],
                              d->pads[1], flip, (const uint8_t *)x_zp, di->x_signed, rten_effective_pad_mode(di));
}

// Load-time staging of a constant MatMulInteger RHS (PackedBMatrix, rten-gemm/src/prepack.rs:19-120; packing/int8.rs:80-249
// keeps the column sums inside the packed image, as here).  Layout: [Kp/16][n][16] signed bytes, then int32[n] column sums.
RTEN_EXPORT size_t rten_hip_gemm_int8_packed_bytes(int32_t k, int32_t n) {
    if (!gemm_b_covered(k, n)) return 0;
    return up256((size_t)n * gemm_kp(k)) + up256((size_t)n * 4);
}

RTEN_EXPORT int32_t rten_hip_gemm_int8_prepack(rten_hip_ctx *ctx, int32_t k, int32_t n, const void *b, int64_t b_rs, int64_t b_cs, int32_t b_signed, void *packed) {
    RTEN_CHECK_CTX(ctx);
    if (!b || !packed) return RTEN_HIP_ERR_INVALID_VALUE;
    if (!gemm_b_covered(k, n)) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "gemm_int8 prepack: shape not covered by the staged kernel (packed_bytes == 0)");
    if (b_rs < 0 || b_cs < 0) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "gemm_int8 prepack: negative strides are not supported");
    const int Kp = gemm_kp(k);
    rten_i8_pack_rows(ctx, b, b_cs, b_rs, n, k, Kp, b_signed ? 0u : 0x80u, (char *)packed, (char *)packed + up256((size_t)n * Kp));
    RTEN_LAUNCH_CHECK(ctx, "i8_pack_rows_kernel launch");
    return RTEN_HIP_OK;
}

RTEN_EXPORT size_t rten_hip_conv2d_int8_packed_bytes(const rten_hip_conv2d_int8_desc *di) {
    if (!di) return 0;
    const ConvGeom g = rten_i8_conv_geom(di);
    return g.ok ? up256((size_t)di->conv.o * g.Kp) + (size_t)di->conv.o * 4 : 0;
}

RTEN_EXPORT int32_t rten_hip_conv2d_int8_prepack(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const void *w, void *packed) {
    RTEN_CHECK_CTX(ctx);
    if (!di || !w || !packed) return RTEN_HIP_ERR_INVALID_VALUE;
    const ConvGeom g = rten_i8_conv_geom(di);
    if (!g.ok) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "conv_int8 prepack: geometry not covered by the staged kernel (packed_bytes == 0)");
    rten_i8_pack_conv_weights(ctx, di, g, w, packed, (char *)packed + up256((size_t)di->conv.o * g.Kp));
    RTEN_LAUNCH_CHECK(ctx, "i8_pack_rows_kernel launch");
    return RTEN_HIP_OK;
}

RTEN_EXPORT size_t rten_hip_conv2d_int8_staged_bytes(const rten_hip_conv2d_int8_desc *di) {
    if (!di || di->x_signed) return 0;
    const ConvGeom g = rten_i8_conv_geom(di);
    return g.ok ? up256(g.img) : 0;
}

RTEN_EXPORT int32_t rten_hip_dynamic_quantize_linear_staged(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const float *x, void *staged,
                                                            float *scale, uint8_t *zero_point, const float *mul_by, float *product) {
    RTEN_CHECK_CTX(ctx);
    if (!di || !x || !staged || !scale || !zero_point || (mul_by && !product)) return RTEN_HIP_ERR_INVALID_VALUE;
    return quantize_staged(ctx, di, x, nullptr, staged, scale, zero_point, one_product(mul_by, product));
}

RTEN_EXPORT int32_t rten_hip_dynamic_quantize_linear_staged_stats(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const float *x, const void *stats,
                                                                  void *staged, float *scale, uint8_t *zero_point, const float *mul_by, float *product) {
    RTEN_CHECK_CTX(ctx);
    if (!di || !x || !stats || !staged || !scale || !zero_point || (mul_by && !product)) return RTEN_HIP_ERR_INVALID_VALUE;
    return quantize_staged(ctx, di, x, stats, staged, scale, zero_point, one_product(mul_by, product));
}

RTEN_EXPORT int32_t rten_hip_dynamic_quantize_linear_staged_products(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const float *x, const void *stats,
                                                                     void *staged, float *scale, uint8_t *zero_point, int32_t count,
                                                                     const float *const *mul_by, float *const *product) {
    RTEN_CHECK_CTX(ctx);
    if (!di || !x || !staged || !scale || !zero_point || count < 0 || (count > 0 && (!mul_by || !product))) return RTEN_HIP_ERR_INVALID_VALUE;
    if (count > kMaxProducts) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "quantize_staged_products: at most 4 scale products per launch");
    ScaleProducts sp = {};
    sp.count = count;
    for (int i = 0; i < count; i++) {
        if (!mul_by[i] || !product[i]) return RTEN_HIP_ERR_INVALID_VALUE;
        sp.mul_by[i] = mul_by[i];
        sp.product[i] = product[i];
    }
    return quantize_staged(ctx, di, x, stats, staged, scale, zero_point, sp);
}

RTEN_EXPORT size_t rten_hip_minmax_stats_bytes(void) { return 2 * dql::kStatSlots * sizeof(unsigned); }

RTEN_EXPORT int32_t rten_hip_minmax_stats_reset(rten_hip_ctx *ctx, void *stats, int32_t count) {
    RTEN_CHECK_CTX(ctx);
    if (!stats || count < 1) return RTEN_HIP_ERR_INVALID_VALUE;
    const int n = count * 2 * dql::kStatSlots;
    hipLaunchKernelGGL(stats_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (unsigned *)stats, count);
    RTEN_LAUNCH_CHECK(ctx, "stats_reset_kernel launch");
    return RTEN_HIP_OK;
}
