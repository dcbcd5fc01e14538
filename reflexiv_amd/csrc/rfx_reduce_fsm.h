// rfx_reduce_fsm.h -- the per-row transition of the two window adjustments of the k-mer reduction stage:
// LeftLongerKmerVariantAdjustment (P/ReflexivDSDynamicKmerRuduction.java :1889-2245) and
// RightLongerKmerVariantAdjustmentAndNeutralization (:1203-1574).  Plain C++, no HIP types: the kernels (rfx_reduce.hip) and a host
// program (tests/reduce_fsm_main.cpp) share it.
//
// Both classes keep at most two pending rows, always the UNMODIFIED rows right before the current one, so the state ahead of row
// i is the number of pending rows, 0, 1 or 2.  From 0 a row becomes pending (-> 1), from 1 too (-> 2); from 2 the rows a = i - 2,
// b = i - 1, c = i decide (rfx_fsm_window): `shift` (a out, b and c pending), `two` (a and b out -- or one of them --, c
// pending) or `three` (all decided, nothing pending).  A row is therefore a map {0,1,2} -> {0,1,2}, six bits, and a partition is
// the inclusive scan of its rows' maps from state 0 plus one flush of what is still pending (rfx_fsm_flush).  The first row of a
// partition ignores what came before it: its map is the constant 1, which also cuts the scan there.
#ifndef RFX_REDUCE_FSM_H
#define RFX_REDUCE_FSM_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RFX_FSM_FN __host__ __device__ inline
#else
#define RFX_FSM_FN inline
#endif

// what the three rows of a window look like (bits of `in`): which are SHORT (key of k1 - 1 bases), which pairs pass
// dynamicSubKmerComparator (the shorter key is a prefix of the longer one), which pairs have equal extensions
enum {
    RFX_FSM_SA = 1, RFX_FSM_SB = 2, RFX_FSM_SC = 4,
    RFX_FSM_PAB = 8, RFX_FSM_PBC = 16, RFX_FSM_PAC = 32,
    RFX_FSM_EAB = 64, RFX_FSM_EBC = 128, RFX_FSM_EAC = 256
};
// emit: bit 0 row a, bit 1 row b, bit 2 row c, written in that order; edit: 0 none, 1 row a takes from row b, 2 row b takes from
// row a (the edited row takes the other's extension and rfx_fsm_edit_marker of its right (left adjustment) / left (right
// adjustment) marker)
struct rfx_fsm_step { unsigned next, emit, edit; };

RFX_FSM_FN int rfx_fsm_edit_marker(int target, int source) { return source < 0 && target >= 0 ? -1 : target; }

// state 2, rows a b c
RFX_FSM_FN rfx_fsm_step rfx_fsm_window(bool right, unsigned in) {
    const bool pab = in & RFX_FSM_PAB, pbc = in & RFX_FSM_PBC, pac = in & RFX_FSM_PAC;
    const bool eab = in & RFX_FSM_EAB, ebc = in & RFX_FSM_EBC, eac = in & RFX_FSM_EAC;
    const rfx_fsm_step shift{2u, 1u, 0u}, two{1u, 3u, 0u};
    const rfx_fsm_step edit_a{1u, right ? 1u : 3u, 1u}, edit_b{1u, right ? 2u : 3u, 2u};      // (the right one drops the shorter row)
    switch (in & 7u) {
    case RFX_FSM_SA | RFX_FSM_SB | RFX_FSM_SC: return two;                                     // :1924 / :1238
    case RFX_FSM_SA | RFX_FSM_SB: return pbc ? shift : two;                                    // S S L  :1935 / :1249
    case RFX_FSM_SA | RFX_FSM_SC: return pab ? edit_b : pbc ? shift : two;                     // S L S  :1969 / :1283
    case RFX_FSM_SA:                                                                           // S L L  :2005 / :1319
        if (pab && pac) return rfx_fsm_step{0u, right && (eab || eac) ? 6u : 7u, 0u};
        return pab ? edit_b : shift;
    case RFX_FSM_SB | RFX_FSM_SC: return pab ? edit_a : two;                                   // L S S  :2062 / :1381
    case RFX_FSM_SB:                                                                           // L S L  :2092 / :1411
        if (pab && pbc) return rfx_fsm_step{0u, right && (eab || ebc) ? 5u : 7u, 0u};
        return pab ? edit_a : pbc ? shift : two;
    case RFX_FSM_SC:                                                                           // L L S  :2138 / :1462
        if (pac && pbc) return rfx_fsm_step{0u, right && (eac || ebc) ? 3u : 7u, 0u};
        return pbc ? shift : two;
    default: return shift;                                                                     // L L L  :2161 / :1490
    }
}

// the end of a partition with two rows pending, x then y: in = RFX_FSM_SA (x short) | RFX_FSM_SB (y short) | RFX_FSM_PAB; `next`
// is unused.  Long then short with a failed prefix test adds NEITHER row (:2213-2229, :1542-1558)
RFX_FSM_FN rfx_fsm_step rfx_fsm_flush(bool right, unsigned in) {
    const bool p = in & RFX_FSM_PAB;
    switch (in & 3u) {
    case RFX_FSM_SA: return p ? rfx_fsm_step{0u, right ? 2u : 3u, 2u} : rfx_fsm_step{0u, 3u, 0u};
    case RFX_FSM_SB: return p ? rfx_fsm_step{0u, right ? 1u : 3u, 1u} : rfx_fsm_step{0u, 0u, 0u};
    default: return rfx_fsm_step{0u, 3u, 0u};
    }
}

// a row's map: bits 2 s .. 2 s + 1 = the state behind the row when s is the state ahead of it
RFX_FSM_FN unsigned rfx_fsm_map(bool partition_start, unsigned next_from_2) { return partition_start ? 0x15u : (1u | (2u << 2) | (next_from_2 << 4)); }
RFX_FSM_FN unsigned rfx_fsm_apply(unsigned map, unsigned s) { return (map >> (2u * s)) & 3u; }
// first f, then g
RFX_FSM_FN unsigned rfx_fsm_compose(unsigned f, unsigned g) {
    return rfx_fsm_apply(g, rfx_fsm_apply(f, 0u)) | (rfx_fsm_apply(g, rfx_fsm_apply(f, 1u)) << 2) | (rfx_fsm_apply(g, rfx_fsm_apply(f, 2u)) << 4);
}
#define RFX_FSM_IDENTITY 0x24u

RFX_FSM_FN unsigned rfx_fsm_popcount3(unsigned m) { return (m & 1u) + ((m >> 1) & 1u) + ((m >> 2) & 1u); }

#endif
