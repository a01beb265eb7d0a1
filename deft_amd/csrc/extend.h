// Flatten metadata of an EXTEND step: R new tokens (1 <= R <= 1024), several per live leaf, each one a query row AND a new
// K/V row.  Token t belongs to leaf row_leaf[t] (query-row index of the leaf in the tree as it stands), rows grouped by
// leaf, and hangs either off the end of the leaf's cached path (parent[t] = -1) or off an earlier token of the same leaf
// (parent[t] = its row index, < t).  Row t attends over path_slots(leaf) + {cache_loc[u] : u is t or an ancestor of t}:
// a chain per leaf is causal extend, a general parent array is draft-tree verification.
//
// Nothing new attends: the kernels below only write the six block arrays the Flatten operator reads
// (deft_flatten_decode_append_*), so stage 1 and the merge run as they are.
//
//   cached keys   the block arrays of the tree itself (tree_plan.h, built without advance: query rows = leaves) are
//                 EXPANDED -- a block's leaf list becomes the concatenation of its leaves' token rows, a leaf's mask bit
//                 its tokens' bits.  Blocks that end without rows are dropped, blocks of more than max_q_len rows are cut
//                 into chunks of max_q_len rows, slots nobody of a chunk sees are dropped from it.  Consecutive blocks with
//                 ONE leaf list (a shared prefix) are emitted chunk-major -- all blocks of chunk 0, then all of chunk 1 --
//                 so that the plan kernels see plain runs of equal query lists, however many chunks there are
//                 (extend_scan_kernel: one workgroup; extend_blocks_kernel: one workgroup per block of the tree)
//   new keys      per leaf, pieces of max_q_len rows; a piece's keys are the leaf's new tokens that are ancestor-or-self of
//                 one of its rows, ascending, cut into 128-slot blocks; each block lists the piece's rows that see one of its
//                 slots.  Consecutive pieces whose keys fit one block are packed greedily while rows <= max_q_len and slots
//                 <= 128 (32 leaves x 1 token: one block).  (extend_new_kernel: one workgroup)
//
// The first part of this file is plain C++ shared with the host (tree.cpp sizes the arrays with the same packing rule);
// the kernels are compiled where DEFT_EXTEND_KERNELS is defined (deft_kernels.hip, behind tree_plan.h).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DEFT_EXT_HD __host__ __device__
#else
#define DEFT_EXT_HD
#endif

namespace deft {

constexpr int EXT_MAX_ROWS = 1024;     // rows of one step (the plan's new-row hash holds as many, plan_kernels.h)
constexpr int EXT_MAX_NEWBLK = 1024;   // new-key blocks of one step (max_q_len 32: at most ~150; a 1024-token chain at max_q_len 1 is refused)
constexpr int EXT_MAX_WORDS = 2048;    // 64-bit words of the key bit sets the new-key kernel keeps in LDS (extend_piece_words)
constexpr int EXT_TILE = 128;
constexpr int EXT_MAX_TBLOCKS = 1 << 16;  // blocks of the tree's own arrays (one bit each in the scan kernel's LDS)
constexpr int EXT_DIMS = 8;            // dims[]: NB, P, NB of the cached part, P of the cached part, error flags
constexpr int EXT_ERR = 4;
// error flags: 1 = row_leaf not ascending / out of range, 2 = parent not in [-1, t) of the same leaf, 4 = output capacity,
//              8 = a list of the tree's arrays longer than 32 / too many pieces, blocks or bit-set words
// A step deft_tree_extend_sizes accepts raises none of them: the host applies the same limits (blocks, words) and refuses there.

// Words of the key bit set of ONE piece of a leaf with M tokens in the step (bit d: token d of the leaf is a key of the piece).
// A leaf has ceil(M / max_q_len) pieces; a step's words are limited to EXT_MAX_WORDS.  With max_q_len >= 16 every step of
// 1024 rows fits: a leaf of M <= 16 tokens takes one word, a longer one ceil(M / 16) ceil(M / 64) <= M^2 / 1024 + 5 M / 64 + 1
// < 1.15 M, under 1200 words over the step.  Below that a long chain on one leaf does not (1024 tokens at max_q_len 4: 256 x 16
// words), and the size query refuses it.
DEFT_EXT_HD inline int extend_piece_words(int M) { return (M + 63) / 64; }

// Greedy packing of the new-key pieces, in order: piece p has rows[p] rows and keys[p] key slots.  A piece of more than
// 128 keys takes ceil(keys / 128) blocks of its own; the others join the open block while rows <= mq and slots <= 128.
// blk / koff / roff: first block, first slot and first row position of the piece in it; blk_len[b]: slots of block b.
// Returns the number of blocks (blk_len holds at most `cap`; more is counted but not written).
DEFT_EXT_HD inline int extend_pack_pieces(int np, const uint16_t* rows, const uint16_t* keys, uint16_t* blk, uint16_t* koff,
                                          uint16_t* roff, uint16_t* blk_len, int cap, int mq) {
    int nb = 0, cur_rows = 0, cur_slots = 0;
    bool open = false;
    for (int p = 0; p < np; ++p) {
        const int r = rows[p], k = keys[p];
        if (k > EXT_TILE) {
            blk[p] = (uint16_t)nb;
            koff[p] = 0;
            roff[p] = 0;
            for (int left = k; left > 0; left -= EXT_TILE, ++nb)
                if (nb < cap) blk_len[nb] = (uint16_t)(left < EXT_TILE ? left : EXT_TILE);
            open = false;
            continue;
        }
        if (!(open && cur_rows + r <= mq && cur_slots + k <= EXT_TILE)) {
            ++nb;
            cur_rows = cur_slots = 0;
            open = true;
        }
        blk[p] = (uint16_t)(nb - 1);
        koff[p] = (uint16_t)cur_slots;
        roff[p] = (uint16_t)cur_rows;
        cur_rows += r;
        cur_slots += k;
        if (nb - 1 < cap) blk_len[nb - 1] = (uint16_t)cur_slots;
    }
    return nb;
}

}  // namespace deft

#ifdef DEFT_EXTEND_KERNELS

namespace deft {

struct ExtStep {
    const int32_t* row_leaf;   // [R] query-row index of the token's leaf, ascending
    const int32_t* parent;     // [R] -1 or an earlier row of the same leaf
    const int32_t* cache_loc;  // [R] pool slot of the token
    int R, nq;
};

struct ExtBlocks {  // six Flatten arrays
    int64_t *q, *cnts, *off, *masks, *kv, *lens;
};

struct ExtScratch {
    int32_t* dims;     // [EXT_DIMS]
    int32_t* tok_off;  // [nq + 1] first row of every leaf
    int32_t* rows;     // [NBT]     expanded rows of every block of the tree's arrays
    int32_t* eoff;     // [NBT + 1] emitted blocks in front of it (as if block-major: right at the first block of a group)
    int32_t* poff;     // [NBT + 1] block_q elements in front of it (the same)
    int32_t* g0;       // [NBT]     first block of its group (consecutive blocks with one leaf list)
    int32_t* g1;       // [NBT]     first block behind the group
};

inline ExtScratch ext_scratch_view(void* base, int nq, int NBT, size_t* bytes) {
    ExtScratch s;
    char* p = static_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t n) {
        int32_t* r = reinterpret_cast<int32_t*>(p + off);
        off = align_up(off + sizeof(int32_t) * n, 256);
        return r;
    };
    s.dims = take(EXT_DIMS);
    s.tok_off = take((size_t)nq + 1);
    s.rows = take((size_t)NBT + 1);
    s.eoff = take((size_t)NBT + 1);
    s.poff = take((size_t)NBT + 1);
    s.g0 = take((size_t)NBT + 1);
    s.g1 = take((size_t)NBT + 1);
    *bytes = off;
    return s;
}

// One workgroup: where every leaf's rows start, the expanded row count of every block of the tree's arrays, the groups of
// consecutive blocks with one leaf list, and the prefix sums that place the expanded blocks.
__global__ __launch_bounds__(1024) void extend_scan_kernel(ExtBlocks T, int NBT, ExtStep st, ExtScratch s, int mq) {
    __shared__ int sWave[16];
    __shared__ int sCarry;
    __shared__ unsigned long long sOpen[EXT_MAX_TBLOCKS / 64];  // bit e: block e opens a group
    const int tid = threadIdx.x;
    if (tid == 0) s.dims[EXT_ERR] = 0;
    for (int w = tid; w < (NBT + 63) / 64; w += 1024) sOpen[w] = 0ull;
    for (int r = tid; r <= st.nq; r += 1024) {  // first row whose leaf is >= r
        int lo = 0, hi = st.R;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (st.row_leaf[mid] < r) lo = mid + 1;
            else hi = mid;
        }
        s.tok_off[r] = lo;
    }
    __threadfence_block();
    __syncthreads();
    for (int t = tid; t < st.R; t += 1024) {
        const int l = st.row_leaf[t];
        if (l < 0 || l >= st.nq || (t > 0 && st.row_leaf[t - 1] > l)) atomicOr(s.dims + EXT_ERR, 1);
    }
    for (int e = tid; e < NBT; e += 1024) {
        const int cnt = (int)T.cnts[e], off = (int)T.off[e];
        int rows = 0;
        bool same = e > 0 && (int)T.cnts[e - 1] == cnt;
        const int poff = e > 0 ? (int)T.off[e - 1] : 0;
        if (cnt > 32 || cnt < 0) {
            atomicOr(s.dims + EXT_ERR, 8);
        } else {
            for (int i = 0; i < cnt; ++i) {
                const int q = (int)T.q[off + i];
                if (q >= 0 && q < st.nq) rows += s.tok_off[q + 1] - s.tok_off[q];
                if (same && T.q[poff + i] != q) same = false;
            }
        }
        s.rows[e] = rows;
        if (!same) atomicOr(&sOpen[e >> 6], 1ull << (e & 63));
    }
    __threadfence_block();
    __syncthreads();
    for (int e = tid; e < NBT; e += 1024) {
        // last opening block at or in front of e (block 0 always opens), first one behind it
        int w = e >> 6;
        unsigned long long x = sOpen[w] & (~0ull >> (63 - (e & 63)));
        while (!x && w > 0) x = sOpen[--w];
        s.g0[e] = x ? 64 * w + 63 - __clzll((long long)x) : 0;
        w = e >> 6;
        x = (e & 63) == 63 ? 0ull : (sOpen[w] & (~0ull << ((e & 63) + 1)));
        const int nw = (NBT + 63) / 64;
        while (!x && w + 1 < nw) x = sOpen[++w];
        const int nxt = x ? 64 * w + __ffsll((long long)x) - 1 : NBT;
        s.g1[e] = nxt < NBT ? nxt : NBT;
    }
    const int nbc = block_exclusive_scan(NBT, [&](int e) { return (s.rows[e] + mq - 1) / mq; }, s.eoff, sWave, &sCarry);
    const int pc = block_exclusive_scan(NBT, [&](int e) { return s.rows[e]; }, s.poff, sWave, &sCarry);
    if (tid == 0) {
        s.dims[2] = nbc;
        s.dims[3] = pc;
    }
}

// One workgroup of 128 threads per block of the tree's arrays: its expansion, chunk by chunk.
__global__ __launch_bounds__(128) void extend_blocks_kernel(ExtBlocks T, int NBT, ExtStep st, ExtScratch s, ExtBlocks o, int mq,
                                                           int NB_cap, int P_cap) {
    __shared__ int sList[32], sN[32], sPre[33], sCnt0;
    const int e = blockIdx.x, k = threadIdx.x;
    if (e >= NBT || s.dims[EXT_ERR]) return;
    const int rows = s.rows[e];
    if (rows <= 0) return;
    const int cnt = (int)T.cnts[e], off = (int)T.off[e], len = (int)T.lens[e];
    if (k < cnt) {
        const int q = (int)T.q[off + k];
        sList[k] = q;
        sN[k] = s.tok_off[q + 1] - s.tok_off[q];
    }
    __syncthreads();
    if (k == 0) {
        int pre = 0;
        for (int i = 0; i < cnt; ++i) {
            sPre[i] = pre;
            pre += sN[i];
        }
        sPre[cnt] = pre;
    }
    __syncthreads();
    const int g0 = s.g0[e], gl = s.g1[e] - g0;
    const int e0 = s.eoff[g0], p0 = s.poff[g0];
    const int chunks = (rows + mq - 1) / mq;
    const bool have = k < len && k < EXT_TILE;
    const int64_t slot = have ? T.kv[(int64_t)e * EXT_TILE + k] : -1;
    const unsigned long long m = have ? (unsigned long long)T.masks[(int64_t)e * EXT_TILE + k] : 0ull;
    const int lane = k & 63, wave = k >> 6;
    for (int c = 0; c < chunks; ++c) {
        const int cnt_c = min(mq, rows - c * mq);
        const int E = e0 + c * gl + (e - g0);
        const int Pq = p0 + gl * mq * c + (e - g0) * cnt_c;
        if (E >= NB_cap || Pq + cnt_c > P_cap) {  // (uniform)
            if (k == 0) atomicOr(s.dims + EXT_ERR, 4);
            return;
        }
        // the leaf's bit becomes the bits of its rows inside this chunk
        unsigned long long nm = 0ull;
        for (int i = 0; i < cnt; ++i)
            if ((m >> i) & 1ull) {
                const int lo = max(sPre[i], c * mq) - c * mq, hi = min(sPre[i + 1], c * mq + cnt_c) - c * mq;
                if (hi > lo) nm |= ((hi - lo >= 64 ? ~0ull : ((1ull << (hi - lo)) - 1ull)) << lo);
            }
        const bool live = nm != 0ull;
        const unsigned long long b = __ballot(live);
        if (wave == 0 && lane == 0) sCnt0 = __popcll(b);
        __syncthreads();
        const int base = wave ? sCnt0 : 0;
        const int pos = base + __popcll(b & ((1ull << lane) - 1ull));
        if (live) {
            o.kv[(int64_t)E * EXT_TILE + pos] = slot;
            o.masks[(int64_t)E * EXT_TILE + pos] = (int64_t)nm;
        }
        // (the second wave's count, through the same word after everybody has read the first wave's)
        __syncthreads();
        if (wave == 1 && lane == 0) sCnt0 = base + __popcll(b);
        __syncthreads();
        const int total = sCnt0;
        if (k >= total) {  // pad like the tree's own arrays
            o.kv[(int64_t)E * EXT_TILE + k] = -1;
            o.masks[(int64_t)E * EXT_TILE + k] = 0;
        }
        if (k < cnt_c) {
            const int X = c * mq + k;
            int i = 0;
            while (i + 1 < cnt && sPre[i + 1] <= X) ++i;
            o.q[Pq + k] = s.tok_off[sList[i]] + (X - sPre[i]);
        }
        if (k == 0) {
            o.cnts[E] = cnt_c;
            o.off[E] = Pq;
            o.lens[E] = total;
        }
        __syncthreads();
    }
}

// One workgroup of 1024 threads, a thread per row: the new-key blocks, placed behind the cached part.
__global__ __launch_bounds__(1024) void extend_new_kernel(ExtStep st, ExtScratch s, ExtBlocks o, int mq, int NB_cap, int P_cap) {
    __shared__ int sWave[16];
    __shared__ int sCarry;
    __shared__ int sTmp[EXT_MAX_ROWS + 1];
    __shared__ int16_t sPar[EXT_MAX_ROWS];
    __shared__ uint16_t sA[EXT_MAX_ROWS], sPid[EXT_MAX_ROWS];
    __shared__ uint16_t pcRow0[EXT_MAX_ROWS], pcRows[EXT_MAX_ROWS], pcM[EXT_MAX_ROWS], pcWoff[EXT_MAX_ROWS], pcK[EXT_MAX_ROWS],
        pcBlk[EXT_MAX_ROWS], pcKoff[EXT_MAX_ROWS], pcRoff[EXT_MAX_ROWS];
    __shared__ unsigned long long sBits[EXT_MAX_WORDS];  // per piece: which tokens of its leaf are keys of the piece
    __shared__ uint16_t sPre[EXT_MAX_WORDS];             // keys in front of every word of sBits, within its piece
    __shared__ uint32_t sRowMask[EXT_MAX_NEWBLK];       // per block: which rows (position roff + row - row0) see a slot of it
    __shared__ uint16_t sBlkLen[EXT_MAX_NEWBLK];
    __shared__ int sNB, sErr;
    const int t = threadIdx.x, R = st.R;
    // (ONE read of the flags the earlier launches left, handed round through LDS: rows of this kernel raise flag 2 below, and a
    //  wave that read the word after that would leave while the others wait at the barriers)
    if (t == 0) sErr = s.dims[EXT_ERR];
    __syncthreads();
    if (sErr || R < 1 || R > EXT_MAX_ROWS) return;
    const bool row = t < R;
    int a = 0, mlen = 0;
    bool first = false;
    if (row) {
        const int l = st.row_leaf[t];
        a = s.tok_off[l];
        mlen = s.tok_off[l + 1] - a;
        int p = st.parent[t];
        if (p != -1 && (p < a || p >= t)) {
            atomicOr(s.dims + EXT_ERR, 2);
            p = -1;
        }
        sPar[t] = (int16_t)p;
        sA[t] = (uint16_t)a;
        first = (t - a) % mq == 0;
    }
    sRowMask[t] = 0u;
    const int NP = block_exclusive_scan(R, [&](int) { return first ? 1 : 0; }, sTmp, sWave, &sCarry);
    int pid = 0;
    if (row) {
        pid = first ? sTmp[t] : sTmp[t] - 1;
        sPid[t] = (uint16_t)pid;
        if (first) {
            pcRow0[pid] = (uint16_t)t;
            pcM[pid] = (uint16_t)mlen;
            pcRows[pid] = (uint16_t)min(mq, a + mlen - t);
        }
    }
    __syncthreads();
    const int NW = block_exclusive_scan(NP, [&](int p) { return extend_piece_words(pcM[p]); }, sTmp, sWave, &sCarry);
    if (NW > EXT_MAX_WORDS) {  // (uniform; deft_tree_extend_sizes refuses such a step: long chains on one leaf at max_q_len < 16)
        if (t == 0) atomicOr(s.dims + EXT_ERR, 8);
        return;
    }
    if (t < NP) pcWoff[t] = (uint16_t)sTmp[t];
    for (int w = t; w < EXT_MAX_WORDS; w += 1024) sBits[w] = 0ull;
    __syncthreads();
    const int woff = row ? pcWoff[pid] : 0;
    // phase A: every row marks itself and its ancestors as keys of its piece
    if (row)
        for (int u = t, n = 0; u >= 0 && n < EXT_MAX_ROWS; u = sPar[u], ++n) {
            const int d = u - a;
            atomicOr(&sBits[woff + (d >> 6)], 1ull << (d & 63));
        }
    __syncthreads();
    if (t < NP) {
        int c = 0;
        const int w0 = pcWoff[t], nw = extend_piece_words(pcM[t]);
        for (int w = 0; w < nw; ++w) {
            sPre[w0 + w] = (uint16_t)c;
            c += __popcll(sBits[w0 + w]);
        }
        pcK[t] = (uint16_t)c;
    }
    __syncthreads();
    if (t == 0) sNB = extend_pack_pieces(NP, pcRows, pcK, pcBlk, pcKoff, pcRoff, sBlkLen, EXT_MAX_NEWBLK, mq);
    __syncthreads();
    const int NBn = sNB;
    if (NBn > EXT_MAX_NEWBLK) {
        if (t == 0) atomicOr(s.dims + EXT_ERR, 8);
        return;
    }
    const bool big = row && pcK[pid] > EXT_TILE;
    const int blk0 = row ? pcBlk[pid] : 0, koff = row ? pcKoff[pid] : 0;
    const int rpos = row ? pcRoff[pid] + (t - pcRow0[pid]) : 0;  // position among the rows the piece's blocks may list
    auto key_index = [&](int u) {  // rank of token u among the keys of this row's piece
        const int d = u - a;
        return (int)sPre[woff + (d >> 6)] + __popcll(sBits[woff + (d >> 6)] & ((1ull << (d & 63)) - 1ull));
    };
    // phase B1: which rows every block lists
    if (row)
        for (int u = t, n = 0; u >= 0 && n < EXT_MAX_ROWS; u = sPar[u], ++n) {
            const int blk = blk0 + (big ? key_index(u) >> 7 : 0);
            atomicOr(&sRowMask[blk], 1u << rpos);
        }
    __syncthreads();
    const int Pn = block_exclusive_scan(NBn, [&](int b) { return __popc(sRowMask[b]); }, sTmp, sWave, &sCarry);
    const int NBc = s.dims[2], Pc = s.dims[3];
    if (NBc + NBn > NB_cap || Pc + Pn > P_cap) {
        if (t == 0) atomicOr(s.dims + EXT_ERR, 4);
        return;
    }
    for (int i = t; i < NBn * EXT_TILE; i += 1024) {
        o.kv[(int64_t)NBc * EXT_TILE + i] = -1;
        o.masks[(int64_t)NBc * EXT_TILE + i] = 0;
    }
    for (int b = t; b < NBn; b += 1024) {
        o.cnts[NBc + b] = __popc(sRowMask[b]);
        o.off[NBc + b] = Pc + sTmp[b];
        o.lens[NBc + b] = sBlkLen[b];
    }
    __threadfence();
    __syncthreads();
    // phase B2: slots, masks and query lists
    if (row)
        for (int u = t, n = 0; u >= 0 && n < EXT_MAX_ROWS; u = sPar[u], ++n) {
            const int idx = key_index(u);
            const int blk = blk0 + (big ? idx >> 7 : 0);
            const int kpos = big ? (idx & 127) : koff + idx;
            const int bit = __popc(sRowMask[blk] & ((1u << rpos) - 1u));
            const int64_t at = (int64_t)(NBc + blk) * EXT_TILE + kpos;
            atomicOr(reinterpret_cast<unsigned long long*>(o.masks + at), 1ull << bit);
            o.kv[at] = st.cache_loc[u];
            o.q[Pc + sTmp[blk] + bit] = t;
        }
    if (t == 0) {
        s.dims[0] = NBc + NBn;
        s.dims[1] = Pc + Pn;
    }
}

}  // namespace deft

#endif  // DEFT_EXTEND_KERNELS
