// Attention states: the merge of two finished (o, lse) pairs.
//
// The STATE of query row r and head h over a key set S is (o, lse): o[D] the normalised attention output in the call's
// element type, lse = ln sum_{i in S} exp(scale q.k_i) in fp32 (natural log, scale included -- the convention of the
// workspace's partial_lse, stage1_np.h); the empty set has o = 0, lse = -inf.  The *_lse entry points return both (the
// stores are in merge.h and prefill.h); this kernel joins the states of two DISJOINT key sets into the state of their union:
//     m = max(lse_a, lse_b);  m = -inf -> (0, -inf);  w_x = exp(lse_x - m), s = w_a + w_b,
//     o = (w_a o_a + w_b o_b) / s in fp32, rounded once;  lse = m + log s.
// A side with lse = -inf has weight exactly 0 and its o is never read into the sum (it may hold anything, NaN included).
//
// A streaming kernel: a group of D / 8 lanes owns one (row, head) pair, each lane eight elements of o_a, o_b and out -- one
// 16-byte access each (VEC), or four 4-byte accesses where a pointer or stride is only 4-byte aligned (the library's output
// contract; a state written by a decode call may be such a view).  An element is read and written by the same lane, so
// out may BE o_a or o_b.  No LDS, no barrier; a capped grid strides over the pairs.
//
// Included by deft_kernels.hip after call.h (the host half uses set_error / check_launch).
#pragma once

namespace deft {

struct MergeStatesParams {
    const e16* o_a;
    const e16* o_b;
    e16* out;
    const float* lse_a;
    const float* lse_b;
    float* lse_out;  // nullable
    int64_t a_st, a_sh, b_st, b_sh, o_st, o_sh;        // elements
    int64_t la_st, la_sh, lb_st, lb_sh, lo_st, lo_sh;  // elements
    int64_t pairs;  // n * Hq
    int Hq;
};

template <bool VEC>
__device__ __forceinline__ uintx4 load_row8(const e16* p) {
    if (VEC) return *reinterpret_cast<const uintx4*>(p);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
    return uintx4{w[0], w[1], w[2], w[3]};
}
template <bool VEC>
__device__ __forceinline__ void store_row8(e16* p, uintx4 v) {
    if (VEC) {
        *reinterpret_cast<uintx4*>(p) = v;
    } else {
        uint32_t* w = reinterpret_cast<uint32_t*>(p);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    }
}

template <class T, int D, bool VEC>
__global__ __launch_bounds__(256) void merge_states_kernel(MergeStatesParams p) {
    using vec8 = typename T::vec8;
    constexpr int LPG = D / 8;  // lanes per (row, head) pair
    const int col = (threadIdx.x % LPG) * 8;
    const int64_t step = (int64_t)gridDim.x * (256 / LPG);
    for (int64_t pair = (int64_t)blockIdx.x * (256 / LPG) + threadIdx.x / LPG; pair < p.pairs; pair += step) {
        const int64_t r = pair / p.Hq, hq = pair - r * p.Hq;
        const float la = p.lse_a[r * p.la_st + hq * p.la_sh], lb = p.lse_b[r * p.lb_st + hq * p.lb_sh];  // (uniform in the group)
        const uintx4 ra = load_row8<VEC>(p.o_a + r * p.a_st + hq * p.a_sh + col);
        const uintx4 rb = load_row8<VEC>(p.o_b + r * p.b_st + hq * p.b_sh + col);
        const float m = fmaxf(la, lb);
        const bool live = m != -INFINITY;
        const float wa = (la == -INFINITY) ? 0.f : __expf(la - m), wb = (lb == -INFINITY) ? 0.f : __expf(lb - m);
        const float s = wa + wb;
        const vec8 xa = __builtin_bit_cast(vec8, ra), xb = __builtin_bit_cast(vec8, rb);
        vec8 y;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            // a side of weight 0 contributes an exact 0, whatever its o holds
            const float fa = wa > 0.f ? wa * T::to_float(xa[e]) : 0.f, fb = wb > 0.f ? wb * T::to_float(xb[e]) : 0.f;
            y[e] = T::from_float(live ? (fa + fb) / s : 0.f);
        }
        store_row8<VEC>(p.out + r * p.o_st + hq * p.o_sh + col, __builtin_bit_cast(uintx4, y));
        if (p.lse_out && col == 0) p.lse_out[r * p.lo_st + hq * p.lo_sh] = live ? m + logf(s) : -INFINITY;
    }
}

template <class T>
static int merge_states_t(const void* o_a, int64_t a_st, int64_t a_sh, const float* lse_a, int64_t la_st, int64_t la_sh,
                          const void* o_b, int64_t b_st, int64_t b_sh, const float* lse_b, int64_t lb_st, int64_t lb_sh, void* out,
                          int64_t o_st, int64_t o_sh, float* lse_out, int64_t lo_st, int64_t lo_sh, int n, int Hq, int D,
                          void* stream) {
    if (!o_a || !o_b || !out || !lse_a || !lse_b) {
        set_error("merge_states: null state pointer (only lse_out may be null)");
        return DEFT_EINVAL;
    }
    if (n < 0 || Hq <= 0) {
        set_error("merge_states: bad geometry n=%d Hq=%d", n, Hq);
        return DEFT_EINVAL;
    }
    if (D != 16 && D != 32 && D != 64 && D != 128) {
        set_error("merge_states: unsupported head_dim %d (supported: 16, 32, 64, 128)", D);
        return DEFT_EUNSUPPORTED;
    }
    auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if (((addr(o_a) | addr(o_b) | addr(out)) & 3u) || ((a_st | a_sh | b_st | b_sh | o_st | o_sh) & 1)) {
        set_error("merge_states: o_a / o_b / out rows must be 4-byte aligned");
        return DEFT_EINVAL;
    }
    if ((addr(lse_a) | addr(lse_b) | addr(lse_out)) & 3u) {
        set_error("merge_states: lse pointers must be 4-byte aligned");
        return DEFT_EINVAL;
    }
    if (n == 0) return DEFT_OK;
    const bool vec = !((addr(o_a) | addr(o_b) | addr(out)) & 15u) && !((a_st | a_sh | b_st | b_sh | o_st | o_sh) & 7);
    MergeStatesParams p{static_cast<const e16*>(o_a), static_cast<const e16*>(o_b), static_cast<e16*>(out), lse_a, lse_b, lse_out,
                        a_st, a_sh, b_st, b_sh, o_st, o_sh, la_st, la_sh, lb_st, lb_sh, lo_st, lo_sh, (int64_t)n * Hq, Hq};
    // a streaming launch: as many workgroups as there is work, capped at 8 per CU's worth with a grid stride beyond
    const int64_t per_wg = 256 / (D / 8);
    const unsigned grid = (unsigned)std::min<int64_t>((p.pairs + per_wg - 1) / per_wg, 2048);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define DEFT_STATES_LAUNCH(DD)                                                                            \
    if (vec) hipLaunchKernelGGL((merge_states_kernel<T, DD, true>), dim3(grid), dim3(256), 0, st, p); \
    else hipLaunchKernelGGL((merge_states_kernel<T, DD, false>), dim3(grid), dim3(256), 0, st, p)
    if (D == 128) { DEFT_STATES_LAUNCH(128); }
    else if (D == 64) { DEFT_STATES_LAUNCH(64); }
    else if (D == 32) { DEFT_STATES_LAUNCH(32); }
    else { DEFT_STATES_LAUNCH(16); }
#undef DEFT_STATES_LAUNCH
    return check_launch("merge_states launch");
}

}  // namespace deft
