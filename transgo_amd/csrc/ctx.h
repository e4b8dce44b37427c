// ctx.h -- host-side context shared by the translation units of libtransgo_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/transgo_hip.h"
#include "board_dev.h"

namespace tg {

struct DevBuf {                       // grow-only device scratch
    void* p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 2 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) return -1;
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct Engine;                        // tree + network state (engine.hip)

// Symmetry-aware evaluation (symmetry.hip; tg_net_set_symmetry).  Context state like the weights: it outlives a weight load, is no
// part of a snapshot, and every buffer below stays unallocated until a forward runs with a mode other than 0.
enum { SYM_NONE = 0, SYM_FIXED = 1, SYM_POSITION = 2, SYM_MEAN8 = 3 };
struct SymState {
    int mode = SYM_NONE;
    uint32_t arg = 0;                 // SYM_FIXED: s; SYM_POSITION: seed
    DevBuf packed;                    // [rows][obs_words] tg_net_predict's float planes, bit-packed (dense rows)
    DevBuf bits;                      // [rows][obs_words] the transformed planes the forward reads
    DevBuf ident;                     // [rows] identity slot table of `bits`
    int ident_rows = 0;               //        rows of it that are filled
    DevBuf sym_of_row;                // [rows] s each row was evaluated under (transform kernel -> back-map kernel)
    DevBuf pol, val, own;             // [rows][A], [rows], [rows][P]: the forward's outputs in the transformed orientation
    // HIP-event timing of the two kernels on the context's stream (tg_prof_enable_symmetry)
    bool prof = false; std::vector<hipEvent_t> ev; std::vector<char> ev_kind; size_t ev_used = 0;
    double transform_ms = 0, backmap_ms = 0; long launches = 0;
    size_t bytes() const { return packed.cap + bits.cap + ident.cap + sym_of_row.cap + pol.cap + val.cap + own.cap; }
    void release() {
        packed.release(); bits.release(); ident.release(); sym_of_row.release(); pol.release(); val.release(); own.release();
        ident_rows = 0;
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear(); ev_kind.clear(); ev_used = 0;
    }
};

// symmetry.hip: the launches behind the wrapper around the forward (net.hip: forward_sym).  All on ctx->stream.
int sym_reserve(tg_ctx* ctx, int rows, int words, int A, int P, bool want_packed);
int sym_pack(tg_ctx* ctx, const float* obs, int rows, int C, int P, int words);                   // float planes -> sym.packed
// rows of `src` (through `slot`; nullptr = dense) -> sym.bits under a per-row s: sel SYM_FIXED: s = arg, SYM_POSITION: sym_of(arg, row)
int sym_transform(tg_ctx* ctx, const uint32_t* src, const int32_t* slot, int rows, int S, int C, int words, int sel, uint32_t arg);
// sym.pol / val / own -> policy / value / own (may be nullptr) in the original orientation; acc 0: store, 1: add, 2: add, then * 0.125f
int sym_backmap(tg_ctx* ctx, float* policy, float* value, float* own, int rows, int S, int acc);

}  // namespace tg

struct tg_ctx {
    tg_config cfg;
    int S = 9, P = 81, A = 82;
    int state_bytes = 48;
    hipStream_t stream = nullptr;
    std::string err;
    tg::RulesCfg rules;
    // env scratch
    tg::DevBuf env_in, env_out, env_act, env_flags, env_u8, env_f32, env_i32, env_rng, env_moves;
    tg::Engine* eng = nullptr;
    tg::SymState sym;
};

#define TG_HIP(ctx, expr)                                                                       \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                     \
            return TG_ERR_HIP;                                                                  \
        }                                                                                       \
    } while (0)

#define TG_FAIL(ctx, code, msg) do { (ctx)->err = (msg); return (code); } while (0)
