// Stage 1 over an fp8 KV pool (OCP e4m3fn codes, one byte per element, per-KV-head fp32 scales), the quantising paged append, and the
// two fused (APP).
//
// Included by deft_kernels.hip after stage1_np.h, whose structure this kernel keeps (read that header first): one workgroup per chunk
// of KV tiles, four waves that are each their own pipeline -- wave w stages keys [32w, 32w+32) of a tile into its private LDS slices
// with global_load_lds_dwordx4 and consumes exactly those rows under its own counted s_waitcnt vmcnt, no barrier between load and
// use -- S^T = K Q^T with the wave's 32 keys on M, P^T staying in registers as the B operand of O^T += V^T P^T, the one-barrier
// epilogue, the full-tile mask skip, the scalar-load descriptor ramp.  It reads the SAME plan records (plan_records.h): a pool row
// is 128 bytes, the host hands the plan builders `byte stride / 2` as the slot stride, so a record's byte offsets are right as they
// stand.  Everything after the fragments is the 16-bit kernel's arithmetic: fp32 scores, P rounded once to T, 16-bit MFMA for both
// products, fp32 normalised partial rows + lse for the unchanged merge.
//
// What is new:
//   * a wave's slice is 32 rows x 128 B = 4 KB of K and 4 KB of V: four DMA instructions each (a DMA moves 8 rows, 8 lanes x 16 B a
//     row) instead of eight.  One KV head per work item -- odd head counts need no second form, a work item keeps ONE O accumulator,
//     and the MFMA count per byte read is what it was; the head-pair form (two heads share a 256-byte stretch) would keep the 16-bit
//     kernel's DMA granules at the price of 128 accumulation registers and a fallback.
//   * fragments are converted on their way from LDS to the MFMA with v_cvt_scalef32_pk_{f16,bf16}_fp8 at scale 1.0: e4m3 -> T is
//     EXACT for both T (3 mantissa bits, the range fits, subnormals included).  The scales never see a 16-bit rounding:
//     k_scale[head] multiplies the fp32 softmax scale of the work item, v_scale[head] the fp32 sum in the epilogue.
//
// Lane <-> element maps (c = lane & 31, h = lane >> 5; tg = lane >> 4, tx = lane & 15):
//   K slice  [32 keys][128 B]; the 16-byte chunk ch of row r sits at position ch ^ ((r >> 1) & 7) (the four 16-lane groups of a
//            ds_read_b128 then hit 16 different 16-byte slots of the 256-byte bank row).
//            S^T, A operand: lane (c, h) reads chunk 2j + h of key row c with ONE ds_read_b128 for the k-step PAIR j = 0..3: bytes
//            0-7 are k-step 2j (d = 32j + 16h + 0..7), bytes 8-15 k-step 2j+1 (d = 32j + 16h + 8..15).  The contraction order over d
//            is permuted against the 16-bit kernel's; the Q fragment of k-step s = 2j + e is therefore Q[c][32j + 16h + 8e ..+7],
//            the 16-byte chunk 4j + 2h + e of the (16-bit) Q row.
//   V slice  [32 keys][128 B]; chunk ch of row r at position ch ^ 2 * (((r >> 1) & 1) | (((r >> 3) & 1) << 1)).
//            O^T, A operand of k-step t (keys 16t..16t+15), column block blk: ds_read_b64_tr_b8.  Per 16-lane group the instruction
//            gathers an [8 rows][16 bytes] block -- lane 2q + pp of the group supplies the address of row q, bytes 8pp..8pp+7 -- and
//            lane tx receives byte column tx, row q in byte q.  Group tg reads rows key(q) = 16t + 4(tg >> 1) + (q & 3) + 8(q >> 2),
//            columns d = 32 blk + 16(tg & 1) + 0..15: lane (c, h) = (16(tg & 1) + tx, tg >> 1) thus holds V[key][32 blk + c] for
//            exactly the keys whose probabilities it holds in score registers 8t .. 8t+7 (keys 16t + 4h + e, e < 4, and
//            16t + 8 + 4h + e - 4): P^T is the B operand as it stands.  A 32-lane half touches 8 rows x 32 bytes: with the XOR
//            above the 32 eight-byte pieces cover one 256-byte bank row exactly.
//
// The fused quantising append (APP = true; the *_decode_append_*_kv8 entry points).  With APP = false the plans are built with
// cache_loc = NULL, no record has bit 63 of a row offset set, and the kernel is the one it was before the parameter existed.  With APP:
//   * pool write: workgroup W-1-bid takes new rows W-1-bid, +W, ...: one thread per 16-byte piece of T -> 8 codes through quant_fp8x8
//     with the head's scale (kv8_append_kernel's function: the same bytes), one 8-byte store to K and to V at cache_loc * pool_ss
//     BYTES.  Nobody reads those pool rows in this launch.
//   * a record built with cache_loc flags this step's rows with bit 63 of rowoff; the low bits are the row's byte offset in the 16-bit
//     k_new / v_new.  Such a row is 256 bytes of T, not 128 bytes of codes: no DMA can stage it.  load_rowoff takes one ballot over the
//     sign of the wave's 32 offsets; a slice without a flagged row runs the instruction stream it always ran.  Otherwise (wave-uniform
//     slow path) all LPT DMA instructions are issued with every lane active, the flagged lanes pointed at the head's first pool row --
//     the counted s_waitcnt vmcnt sees what it always sees -- and at the top of iteration i (rowoff[] still holds tile i's offsets, K(i)
//     and V(i) are issued) every lane loads 32 bytes of T, drains vmcnt(0), quantises, and a flagged lane overwrites the 16
//     bytes its DMA lane wrote (ldsK / ldsV + i * 1024 + lane * 16: chunk kchunk_b / vchunk_b of the row, the swizzle sits in the source
//     chunk); s_waitcnt lgkmcnt(0) before the fragment reads.  The codes that reach the MFMA are the codes the pool receives: the call
//     equals kv_append + the APP = false kernel bit for bit.
//   * hazards: the ds_write is ordered behind the DMA write to the same bytes by the vmcnt(0) that covers that DMA, by nothing else; no
//     exec-masked LDS-DMA; every lane loads (the unflagged ones a piece of new row 0) so that no piece is conditionally defined -- such
//     values are live across the whole tile loop and spill; K pieces, then V pieces: both at once do not fit beside the accumulators.
//   * cost: on a decode step the new row is the last key of every leaf, so the slow path sits at the end of
//     every leaf's work item; it is faster than the separate append on ToT-50 and slower on the north-star step.
#pragma once

namespace deft {

typedef int32_t intx2 __attribute__((ext_vector_type(2)));

struct Kv8Params {
    Stage1Params s;        // k / v: the pool's bytes; kv_sh in bytes (kv_ss is not read: row offsets come from the plan)
    const char* plan;      // [cap+1][PLAN_BYTES], leaders first (np_record_order)
    const int32_t* hdr;    // plan header: hdr[1] = number of chunk leaders
    int mirror;            // capped grids (DYN): workgroup b takes items b, 2W-1-b, 2W+b, ...
    int fast_n;            // workgroups < fast_n request tile 0's offsets before anything else
    const float* k_scale;  // [Hkv] fp32 on the device, or null = all ones
    const float* v_scale;
};

// APP: this step's new rows, for the fused quantising append
struct Kv8AppParams : Kv8Params {
    const int32_t* cache_loc;  // [n_new] pool slots
    const e16* k_new;          // [n_new] rows of T, new_st elements apart, heads contiguous ([Hkv][128])
    const e16* v_new;
    int64_t new_st;
    int64_t pool_ss;           // the pool's slot stride in BYTES (s.kv_ss is the plan builders' 2-byte unit)
    int n_new;
};

// two e4m3 codes (word HI of w) -> two elements of T, exact
template <class T, bool HI>
__device__ __forceinline__ typename T::vec2 cvt_fp8x2(uint32_t w) {
    if constexpr (std::is_same<T, F16>::value) return __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI);
    else return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI);
}
// eight codes (two dwords, byte e = element e) -> one MFMA fragment
template <class T>
__device__ __forceinline__ typename T::vec8 cvt_fp8x8(uint32_t lo, uint32_t hi) {
    union {
        typename T::vec2 p[4];
        typename T::vec8 v;
    } u;
    u.p[0] = cvt_fp8x2<T, false>(lo);
    u.p[1] = cvt_fp8x2<T, true>(lo);
    u.p[2] = cvt_fp8x2<T, false>(hi);
    u.p[3] = cvt_fp8x2<T, true>(hi);
    return u.v;
}

// eight elements of T (one 16-byte piece) -> eight e4m3 codes: the quantisation of kv8_append_kernel (below) and of the fused append
//   code = RNE_e4m3fn(clamp(float(x) / scale[head], -448, +448)); NaN -> a NaN code; +-0 preserved; subnormal codes produced
template <class T>
__device__ __forceinline__ intx2 quant_fp8x8(uintx4 x, float scale) {
    union {
        uintx4 u;
        typename T::vec8 h8;
    } in;
    in.u = x;
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float y = T::to_float(in.h8[e]) / scale;  // true fp32 division
        // the clamp is explicit (v_med3_f32 returns a finite bound for a NaN input: NaN passes by)
        f[e] = (y != y) ? y : __builtin_amdgcn_fmed3f(y, -448.f, 448.f);
    }
    intx2 r;
    r[0] = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    r[0] = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], r[0], true);
    r[1] = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    r[1] = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], r[1], true);
    return r;
}

struct Kv8Smem {
    // per wave 16 KB: its K slice [32][128 B] at +0, its V slice at +4096; in the epilogue the whole 16 KB is the wave's parked
    // O [32 query rows][128 floats] -- nobody else ever touched it, hence ONE barrier as in the 16-bit kernel
    static constexpr int WAVE = 32 * 128 * 4;
    static constexpr int SLICE = 32 * 128;
    static constexpr int Q_OFF = 4 * WAVE;               // Q rows [32][128] 16-bit elements, chunks XOR-ed by (row & 15)
    static constexpr int AUX_OFF = Q_OFF + MQ * 128 * 2;  // per wave 2 slots x 512 B: int64 rowoff[32] | u32 vmask[32] | i32 qsrc[32]
    static constexpr int AUX_SLOT = 512;
    static constexpr int X_OFF = AUX_OFF + 4 * 2 * AUX_SLOT;  // float m[32][4], l[32][4]
    static constexpr int OROW_OFF = X_OFF + 2 * 4 * MQ * 4;   // int32 orow[32] of the leader record (staged twice: one 64-lane DMA)
    static constexpr int BYTES = OROW_OFF + 2 * MQ * 4 + 16;
    static_assert(2 * BYTES <= 160 * 1024, "two workgroups per CU");
};

// NT: K / V rows arrive by non-temporal LDS-DMA; DYN (with NT; GQA launches): the cache policy is the chunk leader's (desc[6]) and a
// capped grid may take its further items in mirrored order -- the rules of stage1_np_kernel, decided by the same host code.
// APP: the fused quantising append (header comment).  With APP = false nothing below differs from the kernel without the parameter.
template <class T, bool NT, bool DYN = false, bool APP = false>
__global__ __launch_bounds__(256, 2) void stage1_kv8_kernel(std::conditional_t<APP, Kv8AppParams, Kv8Params> np) {
    using scalar = typename T::scalar;
    using vec8 = typename T::vec8;
    constexpr int D = 128;
    constexpr int KS = D / 16;
    constexpr int LPT = 32 * D / (64 * 16);  // DMA instructions per wave per K (or V) slice
    static_assert(LPT == 4, "128-byte rows: a DMA instruction moves eight of them");
    using SM = Kv8Smem;
    const Stage1Params& p = np.s;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    const int c = l & 31;
    const int h = l >> 5;
    const int bid = blockIdx.x;
    const int W = (int)gridDim.x;
    const int HP = p.Hkv;

    // ---- fused quantising append (the scheme of stage1_np_kernel): new row j enters the pool through workgroup (grid-1-j) % grid, one
    //      16-byte piece of T per thread -> 8 codes, the bytes kv8_append_kernel writes.  Nobody reads those pool rows in this launch:
    //      the plan flags them and the tile loop takes them from k_new / v_new.
    if constexpr (APP) {
        char* const kw = const_cast<char*>(reinterpret_cast<const char*>(p.k));
        char* const vw = const_cast<char*>(reinterpret_cast<const char*>(p.v));
        for (int copy_job = W - 1 - bid; copy_job < np.n_new; copy_job += W) {
            const int64_t dst = (int64_t)np.cache_loc[copy_job] * np.pool_ss;
            for (int i = tid; i < HP * (D / 8); i += 256) {
                const int hd = i / (D / 8), ch = i - hd * (D / 8);
                const int64_t so = (int64_t)copy_job * np.new_st + hd * D + ch * 8;
                const int64_t d_o = dst + (int64_t)hd * p.kv_sh + ch * 8;  // bytes
                const float ks = np.k_scale ? np.k_scale[hd] : 1.f, vs = np.v_scale ? np.v_scale[hd] : 1.f;
                *reinterpret_cast<intx2*>(kw + d_o) = quant_fp8x8<T>(*reinterpret_cast<const uintx4*>(np.k_new + so), ks);
                *reinterpret_cast<intx2*>(vw + d_o) = quant_fp8x8<T>(*reinterpret_cast<const uintx4*>(np.v_new + so), vs);
            }
        }
    }

    int NI = 0x7fffffff;  // leaders x heads, read with the first item's descriptor
    int item = bid, round = 0;
    auto next_item = [&](int it) __attribute__((always_inline)) {
        if constexpr (DYN) {
            if (np.mirror) {
                int b = bid;
                asm volatile("" : "+s"(b));  // (keeps -1 - bid from being hoisted into a scalar register that lives across the tile loop, where none is free)
                return (++round & 1) ? (round + 1) * W - 1 - b : round * W + b;
            }
        }
        return it + W;
    };
    int rec0 = 0, kvh = 0, fb = 0;
    auto rec_of = [&](int i) { return np.plan + (int64_t)(i == 0 ? rec0 : fb + i - 1) * PLAN_BYTES; };

    // ---- loop-invariant lane constants ------------------------------------------------------------------
    // DMA instruction i of a slice: lane -> row 8i + drow, 16-byte position dpos; it fetches the source chunk position ^ swizzle(row)
    const int dpos = l & 7, drow = l >> 3;
    int kchunk_b[2], vchunk_b[2];  // (by i & 1: the swizzles depend on row bits 1-3 = 4 (i & 1) + (drow >> 1), and on bits 1 and 3)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        kchunk_b[j] = (dpos ^ (4 * j + (drow >> 1))) * 16;
        vchunk_b[j] = (dpos ^ (2 * (((drow >> 1) & 1) | (j << 1)))) * 16;
    }
    const uint32_t ldsK = (uint32_t)w * SM::WAVE;
    const uint32_t ldsV = ldsK + SM::SLICE;
    const uint32_t aux0 = SM::AUX_OFF + (uint32_t)w * 2u * SM::AUX_SLOT;
    // S^T A fragments: key row c, chunk 2j + h at position (2j + h) ^ ((c >> 1) & 7)
    const int krow_b = (int)ldsK + c * D;
    const int kcol_b = (h ^ ((c >> 1) & 7)) * 16;
    // O^T A fragments (8-bit transpose reads, map in the header comment)
    const int tg = l >> 4, tx = l & 15;
    const int tq = tx >> 1;
    const int vtr_row_b = (int)ldsV + (4 * (tg >> 1) + (tq & 3) + 8 * (tq >> 2)) * D + (tx & 1) * 8;
    const int vswz = 2 * (((tq >> 1) & 1) | ((tq >> 2) << 1));
    int vtr_col_b[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) vtr_col_b[blk] = ((2 * blk + (tg & 1)) ^ vswz) * 16;
    // Q rows (16-bit, as in the 16-bit kernel): DMA lane -> row 8w + 4i + qkey, position qpos
    const int qpos = l & 15, qkey = l >> 4;

    const char *kb_pool = nullptr, *vb_pool = nullptr;  // per work item (KV head)
    constexpr int64_t NEW_ROW = (int64_t)1 << 63;

    bool temporal = false;  // (wave-uniform, per work item; DYN)
    int64_t rowoff[LPT];
    bool has_new = false;  // (APP, wave-uniform) some row of the slice whose offsets `rowoff` holds is one of this step's new rows
    auto issue_aux = [&](int i, int slot) {  // 2 DMA: this wave's 32 row offsets; its 32 key masks | the 32 q offsets
        const char* rec = rec_of(i);
        dma4(rec + PLAN_ROWOFF + 32 * w * 8 + 4 * l, aux0 + (uint32_t)slot * SM::AUX_SLOT);
        const char* src2 = (l < 32) ? rec + PLAN_MASK + (32 * w + l) * 4 : rec + PLAN_QSRC + (l - 32) * 4;
        dma4(src2, aux0 + (uint32_t)slot * SM::AUX_SLOT + 256u);
    };
    auto load_rowoff = [&](int slot) {
        const int64_t* ro = reinterpret_cast<const int64_t*>(smem + aux0 + slot * SM::AUX_SLOT);
#pragma unroll
        for (int i = 0; i < LPT; ++i) rowoff[i] = ro[8 * i + drow];
        if constexpr (APP) {  // lane k looks at the sign of row k's offset: one ballot per slice (stage1_np_kernel)
            const int32_t hi = reinterpret_cast<const int32_t*>(ro)[2 * (l & 31) + 1];
            has_new = __builtin_amdgcn_ballot_w64(hi < 0) != 0ull;
        }
    };
    // (APP) the slice holds a new row: a new row is 256 bytes of T, not 128 bytes of codes, so no DMA can stage it.  Every DMA is
    // issued all the same, with every lane active -- the counted waits see the operations they always see -- and the lanes of a new
    // row fetch a piece of the head's first pool row instead; the slow path at the top of the tile's iteration overwrites what they staged.
    auto issue_slice_new = [&](const char* pool, const int (&chunk_b)[2], uint32_t lds) __attribute__((always_inline)) {
        const bool nt = NT && !(DYN && temporal);
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const char* src = pool + (rowoff[i] < 0 ? (int64_t)0 : rowoff[i]) + chunk_b[i & 1];
            if (nt) dma16nt(src, lds + (uint32_t)i * 1024u);
            else dma16(src, lds + (uint32_t)i * 1024u);
        }
    };
    auto issue_k = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of the slice being overwritten
        if constexpr (APP) {
            if (has_new) {
                issue_slice_new(kb_pool, kchunk_b, ldsK);
                return;
            }
        }
        if (NT && !(DYN && temporal)) {
#pragma unroll
            for (int i = 0; i < LPT; ++i) dma16nt(kb_pool + rowoff[i] + kchunk_b[i & 1], ldsK + (uint32_t)i * 1024u);
        } else {
#pragma unroll
            for (int i = 0; i < LPT; ++i) dma16(kb_pool + rowoff[i] + kchunk_b[i & 1], ldsK + (uint32_t)i * 1024u);
        }
    };
    auto issue_v = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (APP) {
            if (has_new) {
                issue_slice_new(vb_pool, vchunk_b, ldsV);
                return;
            }
        }
        if (NT && !(DYN && temporal)) {
#pragma unroll
            for (int i = 0; i < LPT; ++i) dma16nt(vb_pool + rowoff[i] + vchunk_b[i & 1], ldsV + (uint32_t)i * 1024u);
        } else {
#pragma unroll
            for (int i = 0; i < LPT; ++i) dma16(vb_pool + rowoff[i] + vchunk_b[i & 1], ldsV + (uint32_t)i * 1024u);
        }
    };
    auto issue_q = [&]() {  // rows 8w .. 8w+7 of the shared Q buffer, offsets from aux slot 0
        const int32_t* qs = reinterpret_cast<const int32_t*>(smem + aux0 + 256 + 128);
        const char* hb = reinterpret_cast<const char*>(p.q) + (int64_t)kvh * p.G * p.q_sh * 2;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = 8 * w + 4 * i + qkey;
            const int chunk = qpos ^ (row & 15);
            dma16(hb + (int64_t)qs[row] * 2 + chunk * 16, SM::Q_OFF + (uint32_t)(8 * w + 4 * i) * 256u);
        }
    };

    for (bool first = true;; first = false) {
    rec0 = __builtin_amdgcn_readfirstlane(item / HP);
    kvh = __builtin_amdgcn_readfirstlane(item - (item / HP) * HP);
    const char* rec_lead = np.plan + (int64_t)rec0 * PLAN_BYTES;
    const bool spec = first && bid < np.fast_n;  // uniform: the speculative ramp of the workgroups resident at launch
    if (spec) {
        if (w == 0) dma4(rec_lead + PLAN_OROW + 4 * (l & 31), SM::OROW_OFF);
        issue_aux(0, 0);
    }
    // The descriptor, the head's two scales and (once) the leader count by SCALAR loads, all in flight together, one wait.  A null
    // scale pointer means ones: its load reads the descriptor's first word instead (valid memory) and the value is dropped.
    typedef int32_t int8v __attribute__((ext_vector_type(8)));
    int8v dsc;
    uint32_t ks_u, vs_u;
    const float* ksp = np.k_scale ? np.k_scale + kvh : reinterpret_cast<const float*>(rec_lead + PLAN_DESC);
    const float* vsp = np.v_scale ? np.v_scale + kvh : reinterpret_cast<const float*>(rec_lead + PLAN_DESC);
    if (first) {
        int32_t nl;
        asm volatile("s_load_dwordx8 %0, %4, 0x0\n\ts_load_dword %1, %5, 0x0\n\ts_load_dword %2, %6, 0x0\n\ts_load_dword %3, %7, 0x0\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&s"(dsc), "=&s"(nl), "=&s"(ks_u), "=&s"(vs_u)
                     : "s"(rec_lead + PLAN_DESC), "s"(np.hdr + 1), "s"(ksp), "s"(vsp)
                     : "memory");
        NI = nl * HP;
        if (item >= NI) {  // this record slot leads no chunk (speculative read of valid memory): nothing to do
            if (spec) wait_vm<0>();
            break;
        }
    } else {
        asm volatile("s_load_dwordx8 %0, %3, 0x0\n\ts_load_dword %1, %4, 0x0\n\ts_load_dword %2, %5, 0x0\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(dsc), "=&s"(ks_u), "=&s"(vs_u)
                     : "s"(rec_lead + PLAN_DESC), "s"(ksp), "s"(vsp)
                     : "memory");
    }
    const float ksc = np.k_scale ? __uint_as_float(ks_u) : 1.f;
    const float vsc = np.v_scale ? __uint_as_float(vs_u) : 1.f;
    if constexpr (DYN) temporal = NT && __builtin_amdgcn_readfirstlane(dsc[6]) != 0;
    const int n = dsc[4];  // tiles of this chunk (> 0: items only name leaders)
    const int nv = dsc[0];
    fb = dsc[5];
    const uint32_t rowbits = nv >= 32 ? 0xffffffffu : ((1u << nv) - 1u);  // the chunk's live virtual rows
    // |scale| inside the exp2 argument, as in the 16-bit kernel -- times the head's K scale, in fp32: a code c of head h means c * k_scale[h]
    const float sc = fmaxf(fabsf(p.scale_log2e), 1e-30f) * ksc;
    kb_pool = reinterpret_cast<const char*>(p.k) + (int64_t)kvh * p.kv_sh;
    vb_pool = reinterpret_cast<const char*>(p.v) + (int64_t)kvh * p.kv_sh;
    if (!spec) {
        if (w == 0) dma4(rec_lead + PLAN_OROW + 4 * (l & 31), SM::OROW_OFF);
        issue_aux(0, 0);
    }
    // ---- prologue: aux(0) -> Q, K(0), aux(1), V(0) -----------------------------------------------------
    wait_vm<0>();
    load_rowoff(0);
    issue_q();
    issue_k();
    if (n > 1) issue_aux(1, 1);
    issue_v();

    vec8 qf[KS];
    float m_run = -INFINITY, l_run = 0.f;
    floatx16 o[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[b][r] = 0.f;

    for (int i = 0; i < n; ++i) {
        const bool has1 = i + 1 < n, has2 = i + 2 < n;
        const int slot = i & 1;
        if constexpr (APP) {
            // ---- slow path (wave-uniform): tile i holds a new row.  `rowoff` still holds tile i's offsets and K(i), V(i) are both
            //      issued.  A DMA lane of a new row owns the 16-byte piece at lane * 16 of its instruction's 1 KB: 16 codes, chunk
            //      kchunk_b / vchunk_b of the row (the swizzle sits in the SOURCE chunk), i.e. 32 bytes of T at twice that offset.  It
            //      loads them, drains vmcnt(0) -- its loads and every DMA into the two slices, so the ds_write below is ordered behind
            //      the DMA write to the same bytes by the wait that covers that DMA --, quantises with the pool write's function and
            //      scales (the codes that reach the MFMA are the codes the pool receives) and overwrites its piece.
            if (has_new) {
                // (K, then V: sixteen pieces of T in flight per lane at a time -- thirty-two do not fit next to the accumulators)
                auto fix = [&](const char* base, const int (&chunk_b)[2], float scale, uint32_t lds) __attribute__((always_inline)) {
                    uintx4 pn[LPT][2];
#pragma unroll
                    for (int ii = 0; ii < LPT; ++ii) {  // (every lane loads -- the others the same piece of new row 0 -- and only the store is predicated)
                        const char* src = base + (rowoff[ii] < 0 ? rowoff[ii] & ~NEW_ROW : (int64_t)0) + 2 * chunk_b[ii & 1];
                        pn[ii][0] = *reinterpret_cast<const uintx4*>(src);
                        pn[ii][1] = *reinterpret_cast<const uintx4*>(src + 16);
                    }
                    wait_vm<0>();
#pragma unroll
                    for (int ii = 0; ii < LPT; ++ii)
                        if (rowoff[ii] < 0) {
                            const intx2 c0 = quant_fp8x8<T>(pn[ii][0], scale), c1 = quant_fp8x8<T>(pn[ii][1], scale);
                            const uintx4 cq = {(uint32_t)c0[0], (uint32_t)c0[1], (uint32_t)c1[0], (uint32_t)c1[1]};
                            *reinterpret_cast<uintx4*>(smem + lds + ii * 1024 + l * 16) = cq;
                        }
                };
                // (the head's 256 bytes of T inside a new row; the bases are formed here, not kept in registers across the tile loop)
                fix(reinterpret_cast<const char*>(np.k_new) + kvh * (D * 2), kchunk_b, ksc, ldsK);
                fix(reinterpret_cast<const char*>(np.v_new) + kvh * (D * 2), vchunk_b, vsc, ldsV);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the pieces are in LDS before any fragment read of this wave
            }
        }
        // ---- K(i) (and Q) landed: younger than it are aux(i+1) [2] and V(i) [LPT] -----------------------
        if (has1) wait_vm<LPT + 2>();
        else wait_vm<LPT>();
        if (i == 0) {
            lds_barrier();  // Q rows of all four waves visible
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)  // k-step 2j + e: chunk 4j + 2h + e of Q row c
                qf[ks] = *reinterpret_cast<const vec8*>(smem + SM::Q_OFF + c * D * 2 + (((4 * (ks >> 1) + 2 * h + (ks & 1)) ^ (c & 15)) * 16));
            if (p.scale_log2e < 0.f)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) qf[ks] = T::neg(qf[ks]);
        }
        // full tile: every live row sees every one of this wave's 32 keys -- no mask bit needs testing (wave-uniform)
        const uint32_t* masks = reinterpret_cast<const uint32_t*>(smem + aux0 + slot * SM::AUX_SLOT + 256);
        const bool full = __builtin_amdgcn_ballot_w64((masks[l & 31] & rowbits) != rowbits) == 0ull;
        // ---- S^T for this wave's 32 keys: one 16-byte read = 16 codes = two k-steps ------------------------
        floatx16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int j = 0; j < KS / 2; ++j) {
            const uintx4 kk = *reinterpret_cast<const uintx4*>(smem + krow_b + (kcol_b ^ (32 * j)));
            acc = T::mfma(cvt_fp8x8<T>(kk[0], kk[1]), qf[2 * j], acc);
            acc = T::mfma(cvt_fp8x8<T>(kk[2], kk[3]), qf[2 * j + 1], acc);
        }
        if (!full) {  // key masks of this lane's 16 keys (keys 8 g4 + 4 h + j of the wave's 32): masked scores become -inf
            uintx4 m4[4];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) m4[g4] = *reinterpret_cast<const uintx4*>(masks + 8 * g4 + 4 * h);
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = 4 * g4 + j;
                    acc[r] = ((m4[g4][j] >> c) & 1u) ? acc[r] : -INFINITY;
                }
        }
        // row maximum over the UNSCALED scores (the scale is positive: it commutes with the maximum)
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, acc[r]);
        // ---- the K slice is free: next tile's row offsets -> K(i+1), aux(i+2) ---------------------------
        if (has1) {
            wait_vm<LPT>();  // aux(i+1) landed (younger: V(i))
            load_rowoff(slot ^ 1);
            issue_k();
            if (has2) issue_aux(i + 2, slot);
        }
        // ---- wave-private online softmax ------------------------------------------------------------------
        vec8 pb[2];
        {
            const float mxx = max_xor32(mx) * sc;
            const float m_new = fmaxf(m_run, mxx);
            const float msafe = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m_run - msafe);
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const scalar ph = T::from_float(__builtin_amdgcn_exp2f(__builtin_fmaf(acc[r], sc, -msafe)));  // ONE rounding, to nearest even
                pb[r >> 3][r & 7] = ph;
                sum += T::to_float(ph);  // row sums over the ROUNDED probabilities
            }
            sum = sum_xor32(sum);
            l_run = l_run * alpha + sum;
            m_run = m_new;
            if (i > 0 && __builtin_amdgcn_ballot_w64(alpha != 1.f) != 0ull) {
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[b][r] *= alpha;
            }
        }
        // ---- V(i) landed: younger are K(i+1) [LPT] and aux(i+2) [2] -------------------------------------
        if (has2) wait_vm<LPT + 2>();
        else if (has1) wait_vm<LPT>();
        else wait_vm<0>();
        // ---- O^T += V^T P^T: four 32-column blocks x two 16-key steps, one transpose read per MFMA ------
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) {
                typedef __attribute__((address_space(3))) intx2* lds_i2;
                const int vb = vtr_row_b + vtr_col_b[blk] + (16 * t) * D;
                const intx2 vv = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i2)(uintptr_t)(vb));
                o[blk] = T::mfma(cvt_fp8x8<T>((uint32_t)vv[0], (uint32_t)vv[1]), pb[t], o[blk]);
            }
        }
        if (has1) issue_v();  // V(i+1); rowoff still holds tile i+1's offsets
    }

    // ---- epilogue: merge the four waves' (m, l, O), times the head's V scale, one partial row per virtual query row.  ONE barrier:
    //      every wave parks its unscaled O (and m, l) in its own 16 KB and the readers rescale while they sum.
    float* xm = reinterpret_cast<float*>(smem + SM::X_OFF);  // [32 rows][4 waves]: a row's four values are one 16-byte read
    float* xl = xm + 4 * MQ;
    if (h == 0) {
        xm[c * 4 + w] = m_run;
        xl[c * 4 + w] = l_run;
    }
    if (c < nv) {  // [row][128] floats, 16-byte chunk index XOR-ed by the row
        char* dst = smem + ldsK + c * (D * 4);
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k4 = 8 * blk + 2 * j + h;  // d = 32 blk + 8 j + 4 h + (0..3)
                floatx4 v4 = {o[blk][4 * j], o[blk][4 * j + 1], o[blk][4 * j + 2], o[blk][4 * j + 3]};
                *reinterpret_cast<floatx4*>(dst + ((k4 ^ c) & 31) * 16) = v4;
            }
    }
    lds_barrier();
    const int32_t* orow = reinterpret_cast<const int32_t*>(smem + SM::OROW_OFF);
    // wave w sums the 16-byte chunks 8w .. 8w+7 of every row: lane = (row within a group of 8, chunk); the groups' reads are issued
    // unconditionally and only the stores are predicated (stage1_np.h: the epilogue's dependent chains), two groups at a time
    const int k4 = 8 * w + (l & 7);
    const int64_t head_rows = (int64_t)kvh * p.G * p.rows;
#pragma unroll 1
    for (int g0 = 0; 8 * g0 < nv; g0 += 2) {
        floatx4 mw[2], lw[2], b[2][4], res[2];
        float lse[2];
        int orow_q[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int qr = 8 * (g0 + g) + (l >> 3);
            const int off = qr * (D * 4) + ((k4 ^ qr) & 31) * 16;
            mw[g] = *reinterpret_cast<const floatx4*>(xm + qr * 4);
            lw[g] = *reinterpret_cast<const floatx4*>(xl + qr * 4);
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) b[g][ww] = *reinterpret_cast<const floatx4*>(smem + off + ww * SM::WAVE);
            orow_q[g] = orow[qr];
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const float M = fmaxf(fmaxf(mw[g][0], mw[g][1]), fmaxf(mw[g][2], mw[g][3]));
            float L = 0.f;
            floatx4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) {
                const float f = (mw[g][ww] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mw[g][ww] - M);
                L += f * lw[g][ww];
                a += b[g][ww] * f;
            }
            const float inv = L > 0.f ? 1.f / L : 0.f;
            res[g] = (a * vsc) * inv;  // the V scale on the fp32 sum, before the row is normalised
            lse[g] = (L > 0.f) ? (M + __builtin_amdgcn_logf(L)) * LN2 : -INFINITY;
            asm volatile("" : "+v"(res[g]), "+v"(lse[g]));  // (pinned outside the predicated stores)
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int qr = 8 * (g0 + g) + (l >> 3);
            if (qr < nv) {
                const int64_t row = head_rows + orow_q[g];
                *reinterpret_cast<floatx4*>(p.partial_o + row * D + 4 * k4) = res[g];
                if (k4 == 0) p.partial_lse[row] = lse[g];
            }
        }
    }
    {
        const int next = next_item(item);
        if (next >= NI) break;
        lds_barrier();  // every wave is done reading the others' parked rows
        item = next;
    }
    }  // work items
}

// ---------------------------------------------------------------------------
// quantising paged append: one 16-byte piece of a new row (8 elements of T) per thread -> 8 codes (quant_fp8x8), one 8-byte store
// ---------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void kv8_append_kernel(uint8_t* k_base, uint8_t* v_base, int64_t kv_ss, int64_t kv_sh,
                                                          const int32_t* cache_loc, const e16* k_new, const e16* v_new, int64_t new_st,
                                                          int n, int Hkv, int D, const float* k_scale, const float* v_scale) {
    const int ch_per_head = D / 8;
    const int ch_per_tok = Hkv * ch_per_head;
    const int64_t total = (int64_t)n * ch_per_tok;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int tok = (int)(i / ch_per_tok);
        const int rem = (int)(i - (int64_t)tok * ch_per_tok);
        const int hd = rem / ch_per_head;
        const int ch = rem - hd * ch_per_head;
        const int64_t src = (int64_t)tok * new_st + (int64_t)hd * D + ch * 8;
        const int64_t dst = (int64_t)cache_loc[tok] * kv_ss + (int64_t)hd * kv_sh + ch * 8;  // bytes
        const float ks = k_scale ? k_scale[hd] : 1.f, vs = v_scale ? v_scale[hd] : 1.f;
        *reinterpret_cast<intx2*>(k_base + dst) = quant_fp8x8<T>(*reinterpret_cast<const uintx4*>(k_new + src), ks);
        *reinterpret_cast<intx2*>(v_base + dst) = quant_fp8x8<T>(*reinterpret_cast<const uintx4*>(v_new + src), vs);
    }
}

}  // namespace deft
