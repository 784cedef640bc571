// The instantiations of k_rowpass4, as X-macro lists, and the only place that names any: the library can launch nothing else.
//   X(KT, ODD, MODE, EP, NW, SPLIT, Q8)
// Three consumers: rowpass4_inst_*.hip instantiate the lists (KL_RP4_DEFINE: explicit instantiation definitions, compiled in
// parallel with the host-side units: __graft_entry__.compile_library); ctx.hip.h only declares them (KL_RP4_DECLARE: extern
// template); launch_rowpass4_kt (api_loop.hip) fills a table of their addresses (KL_RP4_SLOT) and launches what
// rowpass4_index finds there -- no template-id is written out anywhere.
// How that is checked: the static_assert below proves that rowpass4_index maps the lists one-to-one onto [0, kRowPass4Count):
// every key the index accepts has exactly one kernel, and no kernel is listed that no key reaches.  A list edited without the
// index (or the reverse) does not compile; tests/test_host_cpu.py looks at the built code objects for the rest (each kernel
// compiled once, none outside the lists).
#pragma once

// k <= 224: 8-wave workgroups.  Update pass: whole rows / column-split, each with 16-bit tiles, fp8 tiles, fp8 tiles without
// the numerator's eps; W0 = V.H0^T and loss-only passes: whole rows.
#define KL_RP4_SMALL_OE(X, KT, ODD, EP)                                                                          \
    X(KT, ODD, 0, EP, 8, 0, 0) X(KT, ODD, 0, EP, 8, 1, 0) X(KT, ODD, 0, EP, 8, 0, 1) X(KT, ODD, 0, EP, 8, 1, 1)  \
    X(KT, ODD, 0, EP, 8, 0, 2) X(KT, ODD, 0, EP, 8, 1, 2) X(KT, ODD, 1, EP, 8, 0, 0) X(KT, ODD, 2, EP, 8, 0, 0)
#define KL_RP4_SMALL(X, KT) KL_RP4_SMALL_OE(X, KT, 0, 0) KL_RP4_SMALL_OE(X, KT, 0, 1) KL_RP4_SMALL_OE(X, KT, 1, 0) KL_RP4_SMALL_OE(X, KT, 1, 1)
// 224 < k <= 512: 4-wave workgroups (FUSED order), even KT only
#define KL_RP4_BIG_E(X, KT, EP) X(KT, 0, 0, EP, 4, 0, 0) X(KT, 0, 0, EP, 4, 0, 1) X(KT, 0, 1, EP, 4, 0, 0) X(KT, 0, 2, EP, 4, 0, 0)
#define KL_RP4_BIG(X, KT) KL_RP4_BIG_E(X, KT, 0) KL_RP4_BIG_E(X, KT, 1)

#define KL_RP4_LIST_1(X) KL_RP4_SMALL(X, 1) KL_RP4_SMALL(X, 2) KL_RP4_SMALL(X, 3) KL_RP4_SMALL(X, 4)
#define KL_RP4_LIST_2(X) KL_RP4_SMALL(X, 5) KL_RP4_SMALL(X, 6) KL_RP4_SMALL(X, 7)
#define KL_RP4_LIST_3(X) KL_RP4_BIG(X, 8) KL_RP4_BIG(X, 10) KL_RP4_BIG(X, 12) KL_RP4_BIG(X, 14) KL_RP4_BIG(X, 16)

#define KL_RP4_DEFINE(KT, ODD, MODE, EP, NW, SPLIT, Q8) template __global__ void k_rowpass4<KT, ODD, MODE, EP, NW, SPLIT, Q8>(RowPass4Args);
#define KL_RP4_DECLARE(KT, ODD, MODE, EP, NW, SPLIT, Q8) extern template __global__ void k_rowpass4<KT, ODD, MODE, EP, NW, SPLIT, Q8>(RowPass4Args);
// (inside a function that has `slot`, an array of kRowPass4Count kernel addresses)
#define KL_RP4_SLOT(KT, ODD, MODE, EP, NW, SPLIT, Q8) slot[rowpass4_index(RowPass4Key{KT, ODD, MODE, EP, NW, SPLIT, Q8})] = k_rowpass4<KT, ODD, MODE, EP, NW, SPLIT, Q8>;
#define KL_RP4_KEY(KT, ODD, MODE, EP, NW, SPLIT, Q8) RowPass4Key{KT, ODD, MODE, EP, NW, SPLIT, Q8},

namespace klnmf {

struct RowPass4Key { int kt, odd, mode, ep, nw, split, q8; };

constexpr int kRowPass4Count = 7 * 32 + 5 * 8;

// The dense index of a key: 32 slots per small KT (ODD, EP, then the update pass's SPLIT x Q8 and the two other modes), 8 per big
// KT (EP, then the update pass's Q8 and the two other modes: no ODD, no SPLIT, no NE).  -1: no such kernel.
constexpr int rowpass4_index(const RowPass4Key &k) {
    if (k.odd < 0 || k.odd > 1 || k.ep < 0 || k.ep > 1 || k.split < 0 || k.split > 1 || k.q8 < 0 || k.q8 > 2 || k.mode < 0 || k.mode > 2)
        return -1;
    if (k.mode != 0 && (k.split != 0 || k.q8 != 0)) return -1;
    if (k.kt >= 1 && k.kt <= 7 && k.nw == 8)
        return (k.kt - 1) * 32 + (2 * k.odd + k.ep) * 8 + (k.mode == 0 ? 2 * k.q8 + k.split : 5 + k.mode);
    if (k.kt >= 8 && k.kt <= 16 && k.kt % 2 == 0 && k.nw == 4 && k.odd == 0 && k.split == 0 && k.q8 <= 1)
        return 7 * 32 + (k.kt - 8) / 2 * 8 + k.ep * 4 + (k.mode == 0 ? k.q8 : 1 + k.mode);
    return -1;
}

constexpr RowPass4Key kRowPass4Keys[] = {KL_RP4_LIST_1(KL_RP4_KEY) KL_RP4_LIST_2(KL_RP4_KEY) KL_RP4_LIST_3(KL_RP4_KEY)};

constexpr bool rowpass4_lists_match_index() {
    if (sizeof(kRowPass4Keys) / sizeof(kRowPass4Keys[0]) != kRowPass4Count) return false;
    bool seen[kRowPass4Count] = {};
    for (const RowPass4Key &k : kRowPass4Keys) {
        const int i = rowpass4_index(k);
        if (i < 0 || i >= kRowPass4Count || seen[i] || (k.nw == 8) != (k.kt <= 7)) return false;
        seen[i] = true;
    }
    return true;          // as many distinct slots as there are slots: onto as well
}
static_assert(rowpass4_lists_match_index(), "rowpass4_list.hip.h: the lists and rowpass4_index disagree");

}  // namespace klnmf
