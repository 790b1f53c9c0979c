// What the GroupQueryAttention units share (gqa.hip: the entry point, the prepare launch, the one-workgroup decode kernel and the composed path;
// gqa_split.hip: the decode form that spreads the key range over workgroups): the launch arguments and the device-side lengths.
#pragma once
#include "internal.h"

struct GqaArgs {
    int B, S, H, KV, D, P, T, G; // T = P + S
    int rot, interleaved, max_pos, local;
    int s0, SC; // composed path: the query rows [s0, s0 + SC) of this pass; scores is [B, H, SC, T]
    long long gemv_threads;
    int64_t q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh, bias_sb, bias_sh, bias_sr;
    const float *q, *k, *v, *past_k, *past_v, *cos, *sin, *bias;
    const int32_t *seqlens, *total, *pos;
    float *qr;       // rotated Q [B, S, H, D] (rotary only)
    float *pk, *pv;  // present [B, KV, T, D]
    float *scores;   // composed path: [B, H, S, T]
    float *out;      // [B, S, H * D]
    float scale;
};

static __device__ __forceinline__ void lens(const GqaArgs &p, int b, int &kv_len, int &past_len) {
    long long kv = (long long)p.seqlens[b] + 1;
    kv = kv < 1 ? 1 : (kv > p.T ? p.T : kv);
    long long pl = p.total[0] == p.S ? 0 : kv - p.S;
    pl = pl < 0 ? 0 : (pl > p.P ? p.P : pl);
    kv_len = (int)kv;
    past_len = (int)pl;
}

static __device__ __forceinline__ int past_len_of(const GqaArgs &p, int b) {
    int kv_len, past_len;
    lens(p, b, kv_len, past_len);
    return past_len;
}

static __device__ __forceinline__ void window(const GqaArgs &p, int past_len, int s, int &start, int &lim) {
    lim = past_len + s + 1;
    start = (p.local > 0 && lim > p.local) ? lim - p.local : 0;
}

// gqa_split.hip.  The split decode form's scratch in floats (a function of host-known dims only), and its launches for a call with S == 1, D 64 or 128 and
// a.q already the rotated copy where there is one.  keys_per_workgroup: 0 = the rule, else a positive multiple of 8.  `scratch` holds that many floats.
size_t rten_gqa_split_scratch_elems(const GqaArgs &a);
int32_t rten_gqa_split_launch(rten_hip_ctx *ctx, const GqaArgs &a, int keys_per_workgroup, float *scratch);
// the rule's chunk length for a call's host-known dims, and whether mode 0 prefers the split form to a one-workgroup kernel that fits
int rten_gqa_split_keys(const rten_hip_ctx *ctx, const GqaArgs &a);
bool rten_gqa_split_pays(const rten_hip_ctx *ctx, const GqaArgs &a);

// gqa_prefill.hip.  Whether the fused prefill kernel covers a call's head size and grid (the caller checks that the call is in the blocked order), and its
// launch after gqa_prepare_kernel, with a.q already the rotated copy where there is one.  It needs no scratch.
bool rten_gqa_prefill_covers(const GqaArgs &a);
int32_t rten_gqa_prefill_launch(rten_hip_ctx *ctx, const GqaArgs &a);
