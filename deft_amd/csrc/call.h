// Host-only: the description of one decode call.  The C entry points of deft_kernels.hip (which includes this file after
// Stage1Params, its only translation unit) pack their argument lists into these structs ONCE, and everything behind them -- the
// *_impl functions, the plan builders -- takes the structs.  A struct owns the checks of its fields (the code and the
// deft_last_error text a malformed call gets: tests/test_abi_errors.py) and its part of the kernels' Stage1Params.
#pragma once

namespace deft {

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// q, the K/V pool and the output with their strides (in elements), and the geometry of the call.  The plan builders see the
// geometry alone: plan_geometry() leaves the pointers null.
struct Tensors {
    const void* q;
    int64_t q_st, q_sh;
    const void* k;
    const void* v;
    int64_t kv_ss, kv_sh;
    void* out;
    int64_t o_st, o_sh;
    int nq, Hq, Hkv, D;
    float scale;
    // the *_lse entry points: one fp32 log-sum-exp per (query, head) at lse[q * lse_st + hq * lse_sh] (strides in elements);
    // null and 0 in a plain call
    float* lse = nullptr;
    int64_t lse_st = 0, lse_sh = 0;
    bool lse_call = false;  // an *_lse entry point: a null lse is an error there, not "no log-sum-exp"

    int G() const { return Hq / Hkv; }
    bool heads_ok() const { return Hq > 0 && Hkv > 0 && Hq % Hkv == 0; }
    int check() const {
        if (!q || !k || !v || !out) {
            set_error("null tensor pointer");
            return DEFT_EINVAL;
        }
        if (nq < 0 || !heads_ok()) {
            set_error("bad geometry nq=%d Hq=%d Hkv=%d", nq, Hq, Hkv);
            return DEFT_EINVAL;
        }
        if (!deft_supported(Hq, Hkv, D)) {
            set_error("unsupported geometry Hq=%d Hkv=%d D=%d (head_dim must be 16, 32, 64 or 128)", Hq, Hkv, D);
            return DEFT_EUNSUPPORTED;
        }
        if (!aligned16(q) || !aligned16(k) || !aligned16(v) || (q_st % 8) || (q_sh % 8) || (kv_ss % 8) || (kv_sh % 8)) {
            set_error("q/k/v rows must be 16-byte aligned (pointers and strides multiples of 8 elements)");
            return DEFT_EINVAL;
        }
        if ((reinterpret_cast<uintptr_t>(out) & 3u) || (o_st % 2) || (o_sh % 2)) {
            set_error("out rows must be 4-byte aligned");
            return DEFT_EINVAL;
        }
        if (lse_call && !lse) {
            set_error("null lse (the plain entry point returns no log-sum-exp)");
            return DEFT_EINVAL;
        }
        if (reinterpret_cast<uintptr_t>(lse) & 3u) {
            set_error("lse must be 4-byte aligned");
            return DEFT_EINVAL;
        }
        return DEFT_OK;
    }
    void fill(Stage1Params& p) const {
        p.q = static_cast<const e16*>(q);
        p.q_st = q_st;
        p.q_sh = q_sh;
        p.k = static_cast<const e16*>(k);
        p.v = static_cast<const e16*>(v);
        p.kv_ss = kv_ss;
        p.kv_sh = kv_sh;
        p.Hkv = Hkv;
        p.G = G();
        p.scale_log2e = scale * LOG2E;
    }
};
static Tensors plan_geometry(int Hq, int Hkv, int64_t q_st, int64_t q_sh, int64_t kv_ss) {
    Tensors t{};
    t.Hq = Hq;
    t.Hkv = Hkv;
    t.q_st = q_st;
    t.q_sh = q_sh;
    t.kv_ss = kv_ss;
    return t;
}

// An fp8 (OCP e4m3fn) K/V pool, the *_kv8 entry points: the per-KV-head scales (device pointers, null = ones) and the checks that
// differ from a 16-bit pool's -- Tensors::check() still runs behind them.  Pool strides are in bytes there.
struct Kv8 {
    const float* k_scale;
    const float* v_scale;

    int check(const Tensors& t) const {
        if (t.D != 128) {
            set_error("fp8 KV pool: head_dim %d is not supported (head_dim must be 128; 64, 32 and 16 are not built for fp8 pools)", t.D);
            return DEFT_EUNSUPPORTED;
        }
        if (t.kv_ss % 2) {
            set_error("fp8 KV pool: odd slot stride %lld (the plan addresses rows in 2-byte units)", (long long)t.kv_ss);
            return DEFT_EINVAL;
        }
        if (!aligned16(t.k) || !aligned16(t.v) || (t.kv_ss % 16) || (t.kv_sh % 16)) {
            set_error("fp8 KV pool: base pointers and the slot stride must be 16-byte aligned, the head stride a multiple of 16");
            return DEFT_EINVAL;
        }
        if ((reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale)) & 3u) {
            set_error("fp8 KV pool: k_scale / v_scale must be 4-byte aligned");
            return DEFT_EINVAL;
        }
        return DEFT_OK;
    }
    // what the plan builders and Tensors::check() see: the slot stride in 2-byte units (a record's byte offset is slot * stride * 2)
    static Tensors as_plan_tensors(Tensors t) {
        t.kv_ss /= 2;
        return t;
    }
};

// DeFT-Flatten metadata: the six block arrays, NB blocks, P (query, block) pairs = partial rows per head.
struct FlattenMd {
    const int64_t *block_q, *block_q_cnts, *block_q_offset, *block_bitmasks, *block_kv, *block_lens;
    int NB, P;

    bool ok() const {
        return NB >= 0 && P >= 0 && (NB == 0 || (block_q && block_q_cnts && block_q_offset && block_bitmasks && block_kv && block_lens));
    }
    int check() const {
        if (ok()) return DEFT_OK;
        set_error("bad Flatten metadata (NB=%d P=%d)", NB, P);
        return DEFT_EINVAL;
    }
    int64_t cap(int G) const { return flatten_unit_cap(NB, G); }  // record capacity per KV head
    void fill(Stage1Params& p) const {
        p.block_q = block_q;
        p.block_q_cnts = block_q_cnts;
        p.block_q_offset = block_q_offset;
        p.block_bitmasks = block_bitmasks;
        p.block_kv = block_kv;
        p.block_lens = block_lens;
        p.rows = P;
    }
};

// Partial rows per tile of a Node launch: an entry has at most DEFT_MAX_Q_LEN queries -- and never more than the P (query, entry)
// pairs of the whole call, which is what keeps the scratch of a 100k-token prefix under three branches at a tenth of the
// 32-rows-per-tile figure.  Every sizing function and the launch derive it from P alone, so they agree.
static inline int64_t node_rows_per_tile(int P) { return P <= 0 ? 1 : (P < DEFT_MAX_Q_LEN ? P : DEFT_MAX_Q_LEN); }

// DeFT-Node metadata: the six entry arrays, NE entries, P (query, entry) pairs, total_kv slots in node_kv.
struct NodeMd {
    const int64_t *node_kv, *node_kv_offset, *node_kv_len, *node_q, *node_q_offset, *node_q_len;
    int NE, P;
    int64_t total_kv;
    int rows_per_tile;  // 0: from P; 1: the sequential comparator (one query per entry)

    bool ok() const {
        return NE >= 0 && P >= 0 && total_kv >= 0 && total_kv <= 0x7fffffffLL &&
               (NE == 0 || (node_kv && node_kv_offset && node_kv_len && node_q && node_q_offset && node_q_len));
    }
    int check() const {
        if (ok()) return DEFT_OK;
        set_error("bad Node metadata (NE=%d P=%d total_kv=%lld)", NE, P, (long long)total_kv);
        return DEFT_EINVAL;
    }
    int64_t tiles() const { return node_max_tiles(NE, total_kv); }
    int64_t rows() const { return tiles() * (rows_per_tile > 0 ? rows_per_tile : node_rows_per_tile(P)); }  // every entry has at most that many queries
    PlanView plan(void* base, int G) const { return plan_view(base, tiles() * G, rows()); }
    void fill(Stage1Params& p) const {
        p.node_kv = node_kv;
        p.node_kv_offset = node_kv_offset;
        p.node_kv_len = node_kv_len;
        p.node_q = node_q;
        p.node_q_offset = node_q_offset;
        p.node_q_len = node_q_len;
        p.rows = rows();
    }
};

// Optional fused paged append (deft_*_decode_append_f16): this step's new K/V rows and their pool slots.
struct AppendArgs {
    const e16* k_new = nullptr;
    const e16* v_new = nullptr;
    const int32_t* cache_loc = nullptr;
    int64_t new_st = 0;
    int n_new = 0;
    // fused rotary embedding (optional, with the fused append only): cos | sin row of every new token, [n_new][D] fp32
    const float* cos_sin = nullptr;

    int check(int Hkv, int D) const {
        if (!k_new && !v_new && !cache_loc) return DEFT_OK;
        if (!k_new || !v_new || !cache_loc || n_new < 0 || (new_st % 8) || new_st < (int64_t)Hkv * D || !aligned16(k_new) ||
            !aligned16(v_new)) {
            set_error("bad fused-append arguments (n_new=%d new_stride=%lld)", n_new, (long long)new_st);
            return DEFT_EINVAL;
        }
        return DEFT_OK;
    }
};

// The *_append_* entry points: all three of k_new, v_new and cache_loc, or the call is refused (check() looks at the rest
// once the tensors are known to be sound).
static int make_append(AppendArgs& ap, const int32_t* cache_loc, const void* k_new, const void* v_new, int64_t new_st, int n_new) {
    if (!k_new || !v_new || !cache_loc) {
        set_error("fused append needs k_new, v_new and cache_loc");
        return DEFT_EINVAL;
    }
    ap.k_new = static_cast<const e16*>(k_new);
    ap.v_new = static_cast<const e16*>(v_new);
    ap.cache_loc = cache_loc;
    ap.new_st = new_st;
    ap.n_new = n_new;
    return DEFT_OK;
}
// ... with the fused rotary embedding (the *_rope_append_* entry points): NeoX pairing over the whole head, head_dim 128 (the
// tile-parallel kernel), token-major q so that a virtual row's query index is its element offset / q_stride_tok.
static int make_append(AppendArgs& ap, const int32_t* cache_loc, const void* k_new, const void* v_new, int64_t new_st, int n_new,
                       const float* cos_sin_rows, int rotary_dim, int is_neox_style, const Tensors& t) {
    if (int rc = make_append(ap, cache_loc, k_new, v_new, new_st, n_new)) return rc;
    if (!cos_sin_rows || !aligned16(cos_sin_rows)) {
        set_error("bad fused-rope arguments (cos_sin_rows: [n_new][head_dim] fp32, 16-byte aligned)");
        return DEFT_EINVAL;
    }
    if (t.D != 128 || rotary_dim != t.D || !is_neox_style) {
        set_error("fused rope: head_dim 128, rotary_dim == head_dim, NeoX pairing (got D=%d rotary_dim=%d neox=%d); "
                  "use deft_rope_qk_f16 + the append entry point", t.D, rotary_dim, is_neox_style);
        return DEFT_EUNSUPPORTED;
    }
    if (t.q_st <= 0 || t.q_st > 0x7fffffffLL || (int64_t)(t.Hq - 1) * t.q_sh + t.D > t.q_st || t.q_sh < 0) {
        set_error("fused rope needs token-major q (q_stride_tok=%lld q_stride_head=%lld)", (long long)t.q_st, (long long)t.q_sh);
        return DEFT_EUNSUPPORTED;
    }
    ap.cos_sin = cos_sin_rows;
    return DEFT_OK;
}
// What a plan builder takes of the append: the slots of this step's new rows and their stride.
static AppendArgs plan_append(const int32_t* cache_loc, int n_new, int64_t new_st) {
    AppendArgs ap;
    ap.cache_loc = cache_loc;
    ap.n_new = cache_loc ? n_new : 0;
    ap.new_st = new_st;
    return ap;
}

// The caller's scratch: an optional prebuilt plan, the workspace (carve(), common.h) and the stream.
struct Scratch {
    const void* plan;
    void* workspace;
    size_t workspace_bytes;
    void* stream;

    hipStream_t st() const { return static_cast<hipStream_t>(stream); }
    int check() const {
        if (workspace) return DEFT_OK;
        set_error("null workspace");
        return DEFT_EINVAL;
    }
    int holds(const Workspace& ws) const {
        if (workspace_bytes >= ws.bytes) return DEFT_OK;
        set_error("workspace too small: %zu < %zu", workspace_bytes, ws.bytes);
        return DEFT_EWORKSPACE;
    }
};
// A window plan (window.h): this step's counts on the device, the query chunking and the overflow tiles with their table.
struct WindowArgs {
    int32_t* dims;
    int nq, max_q_len, win_tiles;
    int32_t* win_tab;
    bool ok(int Hq, int Hkv) const { return dims && win_tab && win_tiles >= 1 && deft_window_supported(nq, max_q_len, Hq, Hkv); }
};
static int plan_holds(size_t plan_bytes, size_t need) {
    if (plan_bytes >= need) return DEFT_OK;
    set_error("plan buffer too small: %zu < %zu", plan_bytes, need);
    return DEFT_EWORKSPACE;
}

}  // namespace deft
