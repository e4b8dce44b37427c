// pass_alive_dev.h -- pass-alive groups and territory (Benson's algorithm), one wavefront per board.
//
// transgo_amd/pass_alive.py is the definition.  For each colour X: chains = X's groups, regions = the 4-connected components of the
// points without an X stone.  A region is vital to a chain if it has an empty point and all of its empty points are liberties of the
// chain; chains with fewer than two live vital regions die, regions touching a dead chain die, to the fixed point.  Surviving
// chains are pass-alive (+-2); a surviving region with at most one point that has no X stone next to it is territory (+-1).
//
// 9x9: no LDS at all.  Every lane grows the component of each of its own points (a chain for an X stone, a region otherwise) as an
// 81-bit board in registers, exactly like label_groups(); vitality is a subset test of two such boards, the chain <-> region
// relation lives in per-lane boards of region representatives (lowest point), and one round of the fixed point is two ballots.
// 19x19: LDS min-label propagation (label_groups() over the predicate "X stone or not"), the region's candidate chains taken at its
// lowest empty point and narrowed by the other empty points with atomicAnd, vital counts by atomicAdd, dead chains spread to the
// regions they touch by atomicOr.  Its tables are the kernel's own (PaLds); WaveLds is unchanged.
#pragma once
#include "board_dev.h"

namespace tg {

template <int S> struct PaLds {                    // 19x19 only, indexed by component label (= its lowest point: chains and regions never share one)
    static constexpr int N = S == 9 ? 1 : Geo<S>::PPAD + 64;
    uint32_t lowe[N];      // region: its lowest empty point (kNone: none)
    uint32_t mask[N];      // region: bit d set = the chain at neighbour d of lowe is next to every empty point so far
    uint32_t vit[N];       // chain: live regions vital to it (recounted every round)
    uint32_t dead[N];      // chain or region: 1 = dead
    uint32_t inter[N];     // region: points without an X stone next to them
};

__device__ __forceinline__ uint64_t pa_bcast64(uint64_t v, int src) {      // lane src's value (src wave-uniform)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// One colour at 9x9: x = its stones, emp = the empty points.  sgn[k] = 2 pass-alive stone, 1 territory, 0 neither, for the own points.
__device__ __forceinline__ void pass_alive_colour9(const BoardWave<9>& bw, const B81 x, const B81 emp, int* sgn) {
    constexpr int NW = 2;
    constexpr uint64_t ALL_HI = 0x1FFFFull;
    const int lane = bw.lane;
    const B81 notx{~x.lo, ~x.hi & ALL_HI};
    bool isx[NW], valid[NW];
    B81 comp[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        valid[k] = bw.pt[k] < 81;
        isx[k] = valid[k] && (((k == 0 ? x.lo : x.hi) >> lane) & 1);
        comp[k].lo = (valid[k] && k == 0) ? 1ull << lane : 0ull;
        comp[k].hi = (valid[k] && k == 1) ? 1ull << lane : 0ull;
    }
    for (int it = 0; it < 82; ++it) {                                  // a board only grows and has 81 bits
        bool ch = false;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            B81 n = b81_dilate(comp[k]);
            n.lo &= isx[k] ? x.lo : notx.lo; n.hi &= isx[k] ? x.hi : notx.hi;
            ch |= (n.lo != comp[k].lo) | (n.hi != comp[k].hi);
            comp[k] = n;
        }
        if (!__any(ch)) break;
    }
    // region representatives (lowest point of the region), and per chain lane the representatives of the regions vital to its chain
    B81 dl[NW], vm[NW];
    bool rep[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int low = comp[k].lo ? __ffsll((long long)comp[k].lo) - 1 : 63 + __ffsll((long long)comp[k].hi);
        rep[k] = valid[k] && !isx[k] && low == bw.pt[k];
        dl[k] = b81_dilate(comp[k]);
        vm[k].lo = 0; vm[k].hi = 0;
    }
    B81 reps{ballot64(rep[0]), ballot64(rep[1])};
    int nchain = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int low = comp[k].lo ? __ffsll((long long)comp[k].lo) - 1 : 63 + __ffsll((long long)comp[k].hi);
        nchain += __popcll(ballot64(isx[k] && low == bw.pt[k]));
    }
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        uint64_t m = w == 0 ? reps.lo : reps.hi;
        while (m) {                                                    // at most 81 representatives
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            const uint64_t elo = pa_bcast64(comp[w].lo, l) & emp.lo, ehi = pa_bcast64(comp[w].hi, l) & emp.hi;
            if ((elo | ehi) == 0) continue;                            // a region without an empty point is vital to nothing
#pragma unroll
            for (int k = 0; k < NW; ++k)
                if (isx[k] && ((elo & ~dl[k].lo) | (ehi & ~dl[k].hi)) == 0) { if (w == 0) vm[k].lo |= 1ull << l; else vm[k].hi |= 1ull << l; }
        }
    }
    bool live[NW];                                                     // own point's chain or region is live
#pragma unroll
    for (int k = 0; k < NW; ++k) live[k] = valid[k];
    B81 liverep = reps;
    for (int it = 0; it <= nchain; ++it) {                             // every round but the last kills a chain
        bool ch = false;
#pragma unroll
        for (int k = 0; k < NW; ++k)
            if (isx[k] && live[k] && __popcll(vm[k].lo & liverep.lo) + __popcll(vm[k].hi & liverep.hi) < 2) { live[k] = false; ch = true; }
        const B81 deadx{ballot64(isx[0] && !live[0]), ballot64(isx[1] && !live[1])};
#pragma unroll
        for (int k = 0; k < NW; ++k)
            if (valid[k] && !isx[k] && live[k] && ((dl[k].lo & deadx.lo) | (dl[k].hi & deadx.hi))) live[k] = false;
        liverep.lo = ballot64(rep[0] && live[0]); liverep.hi = ballot64(rep[1] && live[1]);
        if (!__any(ch)) break;
    }
    const B81 nearx = b81_dilate(x);
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int inter = __popcll(comp[k].lo & ~nearx.lo) + __popcll(comp[k].hi & ~nearx.hi);
        sgn[k] = !valid[k] || !live[k] ? 0 : isx[k] ? 2 : inter <= 1 ? 1 : 0;
    }
}

// One colour at 19x19.  X = kBlack or kWhite; rc[k] = the real colours of the own points.  Clobbers bw.col / L->col / L->lab.
template <int S>
__device__ __forceinline__ void pass_alive_colour_lds(BoardWave<S>& bw, PaLds<S>* T, const uint8_t* rc, int X, int* sgn) {
    using G = Geo<S>;
    constexpr int NW = G::NW;
    bool isx[NW], valid[NW];
    uint32_t lb[NW];
    // components of "X stone" and of "no X stone" in one propagation: label_groups(false) joins equal colours
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        valid[k] = bw.pt[k] < G::P;
        isx[k] = valid[k] && rc[k] == X;
        bw.col[k] = (uint8_t)(!valid[k] ? kWall : isx[k] ? kBlack : kWhite);
    }
    bw.publish_colors();
    bw.label_groups(false);
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        lb[k] = valid[k] ? (uint32_t)bw.L->lab[bw.pt[k]] : kNone;
        T->lowe[bw.pt[k]] = kNone; T->mask[bw.pt[k]] = 0xFu; T->vit[bw.pt[k]] = 0; T->dead[bw.pt[k]] = 0; T->inter[bw.pt[k]] = 0;
    }
    __syncthreads();
    // the chains next to each own point that holds no X stone (kNone: no such neighbour in that direction)
    uint16_t nbc[NW][4];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        bool near = false;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            nbc[k][d] = (uint16_t)kNone;
            if (!valid[k] || isx[k] || !(bw.nbv[k] >> d & 1)) continue;
            const int q = bw.pt[k] + BoardWave<S>::nb_off(d);
            if (bw.L->col[q] == kBlack) { nbc[k][d] = bw.L->lab[q]; near = true; }
        }
        if (valid[k] && !isx[k]) {
            if (rc[k] == kEmpty) atomicMin(&T->lowe[lb[k]], (uint32_t)bw.pt[k]);
            if (!near) atomicAdd(&T->inter[lb[k]], 1u);
        }
    }
    __syncthreads();
    // candidates = the chains around the region's lowest empty point; every empty point strikes those it is not a liberty of
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        if (!valid[k] || isx[k] || rc[k] != kEmpty) continue;
        const int le = (int)T->lowe[lb[k]];
        const int lx = le % S, ly = le / S;
        uint32_t m = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const bool on = d == 0 ? lx > 0 : d == 1 ? ly > 0 : d == 2 ? lx < S - 1 : ly < S - 1;
            if (!on) continue;
            const int q = le + BoardWave<S>::nb_off(d);
            if (bw.L->col[q] != kBlack) continue;
            const uint16_t c = bw.L->lab[q];
            if (c == nbc[k][0] || c == nbc[k][1] || c == nbc[k][2] || c == nbc[k][3]) m |= 1u << d;
        }
        atomicAnd(&T->mask[lb[k]], m);
    }
    __syncthreads();
    // region representatives keep the (distinct) chains their region is vital to
    uint16_t vl[NW][4];
    bool rrep[NW], crep[NW];
    int nchain = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        rrep[k] = valid[k] && !isx[k] && lb[k] == (uint32_t)bw.pt[k];
        crep[k] = isx[k] && lb[k] == (uint32_t)bw.pt[k];
        nchain += __popcll(ballot64(crep[k]));
#pragma unroll
        for (int d = 0; d < 4; ++d) vl[k][d] = (uint16_t)kNone;
        if (!rrep[k]) continue;
        const int le = (int)T->lowe[lb[k]];
        if (le == (int)kNone) continue;                                // no empty point: vital to nothing
        const uint32_t m = T->mask[lb[k]];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            if (!(m >> d & 1)) continue;                               // (a set bit implies the neighbour is on the board and an X stone)
            const uint16_t c = bw.L->lab[le + BoardWave<S>::nb_off(d)];
            bool dup = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < d && vl[k][e] == c) dup = true;
            if (!dup) vl[k][d] = c;
        }
    }
    for (int it = 0; it <= nchain; ++it) {                             // every round but the last kills a chain
#pragma unroll
        for (int k = 0; k < NW; ++k) T->vit[bw.pt[k]] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            if (!rrep[k] || T->dead[lb[k]]) continue;
#pragma unroll
            for (int d = 0; d < 4; ++d) if (vl[k][d] != (uint16_t)kNone) atomicAdd(&T->vit[vl[k][d]], 1u);
        }
        __syncthreads();
        bool ch = false;
#pragma unroll
        for (int k = 0; k < NW; ++k)
            if (crep[k] && !T->dead[lb[k]] && T->vit[lb[k]] < 2) { T->dead[lb[k]] = 1; ch = true; }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            if (!valid[k] || isx[k]) continue;
            bool hit = false;
#pragma unroll
            for (int d = 0; d < 4; ++d) if (nbc[k][d] != (uint16_t)kNone && T->dead[nbc[k][d]]) hit = true;
            if (hit) atomicOr(&T->dead[lb[k]], 1u);
        }
        __syncthreads();
        if (!__any(ch)) break;
    }
#pragma unroll
    for (int k = 0; k < NW; ++k)
        sgn[k] = !valid[k] || T->dead[lb[k]] ? 0 : isx[k] ? 2 : T->inter[lb[k]] <= 1 ? 1 : 0;
    __syncthreads();
}

// status[k] for the own points of `st`: +2 / +1 Black pass-alive stone / territory, -2 / -1 White, 0 neither.  All lanes call it
// together.  T is only read at 19x19.  Clobbers the wave's loaded colours and labels.
template <int S>
__device__ __forceinline__ void pass_alive(BoardWave<S>& bw, PaLds<S>* T, const BoardState<S>& st, int8_t* status) {
    using G = Geo<S>;
    int sb[G::NW], sw[G::NW];
    if constexpr (S == 9) {
        constexpr uint64_t ALL_HI = 0x1FFFFull;
        const B81 blk{st.bb[0][0], st.bb[0][1] & ALL_HI}, wht{st.bb[1][0], st.bb[1][1] & ALL_HI};
        const B81 emp{~(blk.lo | wht.lo), ~(blk.hi | wht.hi) & ALL_HI};
        pass_alive_colour9(bw, blk, emp, sb);
        pass_alive_colour9(bw, wht, emp, sw);
    } else {
        uint8_t rc[G::NW];
#pragma unroll
        for (int k = 0; k < G::NW; ++k) {
            int c = kWall;
            if (bw.pt[k] < G::P) c = ((st.bb[0][k] >> bw.lane) & 1) ? kBlack : ((st.bb[1][k] >> bw.lane) & 1) ? kWhite : kEmpty;
            rc[k] = (uint8_t)c;
        }
        pass_alive_colour_lds<S>(bw, T, rc, kBlack, sb);
        pass_alive_colour_lds<S>(bw, T, rc, kWhite, sw);
    }
#pragma unroll
    for (int k = 0; k < G::NW; ++k) status[k] = (int8_t)(sb[k] - sw[k]);
}

// The pass-alive-aware area: owner[k] (1 black, 2 white, 3 dame, as tromp_taylor gives it) overridden where the status is not 0;
// returns #Black - #White (raw, before komi); *is_settled = no point of the board has status 0.
template <int S>
__device__ __forceinline__ float pass_alive_area(BoardWave<S>& bw, PaLds<S>* T, const BoardState<S>& st, int8_t* status, uint8_t* owner,
                                                 bool* is_settled) {
    using G = Geo<S>;
    pass_alive<S>(bw, T, st, status);
    (void)tromp_taylor(bw, st, owner);
    int nb = 0, nw = 0, nz = 0;
#pragma unroll
    for (int k = 0; k < G::NW; ++k) {
        const bool v = bw.pt[k] < G::P;
        if (status[k] > 0) owner[k] = 1;
        else if (status[k] < 0) owner[k] = 2;
        nb += __popcll(ballot64(v && owner[k] == 1));
        nw += __popcll(ballot64(v && owner[k] == 2));
        nz += __popcll(ballot64(v && status[k] == 0));
    }
    *is_settled = nz == 0;
    return (float)(nb - nw);
}

}  // namespace tg
