// What the opset-23 Attention units share (attention_kv.hip: the entry point, the one-workgroup decode kernel and the composed path; attention_split.hip:
// the decode form that spreads the key range over workgroups): the launch arguments and the score modification, moved here from attention_kv.hip unchanged.
#pragma once
#include "internal.h"

struct AttnArgs {
    int B, Hq, Hkv, G, Sq, Skv, P, T, D, Dv; // T = P + Skv
    int causal, mask_kind;                   // mask_kind: RTEN_HIP_ATTN_MASK_*
    int s0, SC;                              // composed path: the query rows [s0, s0 + SC) of this pass; scores is [B, Hq, SC, T]
    long long gemv_threads;
    int64_t q_sb, q_sh, q_ss, k_sb, k_sh, k_ss, v_sb, v_sh, v_ss, o_sb, o_sh, o_ss, m_sb, m_sh, m_sq, m_st;
    const float *q, *k, *v, *past_k, *past_v;
    const void *mask;      // float or int32, by mask_kind
    const int32_t *nonpad; // [B] or NULL
    float *pk, *pv;        // present [B, Hkv, T, D] / [B, Hkv, T, Dv]; NULL in the decode kernels: not stored
    float *scores, *out;
    float scale;
};

static constexpr float NEG_INF = -__builtin_inff();

// nonpad_kv_seqlen[b] clamped into [0, T], or -1 when the input is absent
static __device__ __forceinline__ int nonpad_of(const AttnArgs &p, int b) {
    if (!p.nonpad) return -1;
    const int n = p.nonpad[b];
    return n < 0 ? 0 : (n > p.T ? p.T : n);
}

// the first masked column of row s by steps 2 and 3 of the score modification (T: none)
static __device__ __forceinline__ int masked_from(const AttnArgs &p, int np, int s) {
    if (p.causal) {
        const long long from = (long long)(np >= 0 ? np - p.Sq : p.P) + s + 1;
        return (int)(from < 0 ? 0 : (from > p.T ? p.T : from));
    }
    return np >= 0 ? np : p.T;
}

// steps 1-3 on one score; mrow = the mask's row (b, h, s), already offset
static __device__ __forceinline__ float modified_at(const AttnArgs &p, float o, const void *mrow, int64_t at, int t, int from) {
    if (p.mask_kind == RTEN_HIP_ATTN_MASK_FLOAT) o = o + ((const float *)mrow)[at];
    else if (p.mask_kind == RTEN_HIP_ATTN_MASK_BOOL && ((const int32_t *)mrow)[at] == 0) o = NEG_INF;
    return t >= from ? NEG_INF : o;
}
static __device__ __forceinline__ float modified(const AttnArgs &p, float o, const void *mrow, int t, int from) {
    return modified_at(p, o, mrow, t * p.m_st, t, from); // (`at` apart: attention_prefill.hip forms the element offset itself)
}

static __device__ __forceinline__ const void *mask_row(const AttnArgs &p, int b, int h, int s) {
    const int64_t at = b * p.m_sb + h * p.m_sh + s * p.m_sq;
    return p.mask_kind == RTEN_HIP_ATTN_MASK_FLOAT ? (const void *)((const float *)p.mask + at) : (const void *)((const int32_t *)p.mask + at);
}

// attention_split.hip.  Whether the split decode form takes a call's shapes (the caller has checked one query row and the gemv order): D and Dv each 64 or
// 128, at most 512 query heads per KV head.  Its launches; keys_per_workgroup: 0 = the rule, else a positive multiple of 8.  Scratch comes from
// rten_aux_scratch, a function of host-known dims only.
bool rten_attn_split_covers(const AttnArgs &a);
int32_t rten_attn_split_launch(rten_hip_ctx *ctx, const AttnArgs &a, int keys_per_workgroup);
// the rule's chunk length for a call's dims, and whether mode 0 prefers the split form to a one-workgroup kernel that covers the call
int rten_attn_split_keys(const rten_hip_ctx *ctx, const AttnArgs &a);
bool rten_attn_split_pays(const rten_hip_ctx *ctx, const AttnArgs &a);

// attention_prefill.hip.  Whether the fused prefill kernel takes a call's shapes (the caller has checked that the call is not a one-row call in the gemv
// order): D == Dv in {64, 128}.  Its launch: kc and vc are K and V as contiguous [B, Hkv, T, D], 16-byte aligned (the inputs read in place, present or
// scratch, as on the composed path).  It allocates nothing.
bool rten_attn_prefill_covers(const AttnArgs &a);
int32_t rten_attn_prefill_launch(rten_hip_ctx *ctx, const AttnArgs &a, const float *kc, const float *vc);
