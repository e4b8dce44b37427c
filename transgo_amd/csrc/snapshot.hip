// snapshot.hip -- tg_sp_snapshot_size / tg_sp_snapshot / tg_sp_restore: a running self-play engine as one flat byte buffer.
//
// A snapshot is legal at a MOVE BOUNDARY: no evaluation batch pending and no game inside a search (the state between tg_sp_play +
// tg_sp_expand_roots and the next tg_sp_begin_move).  It holds everything that decides the engine's future behaviour and its
// counters -- GameCtl[G], PoolCtl, the free ring, the RNG streams, the counters, the per-game move counts, the games a harvest
// has not taken yet, the device-side game record -- and the trees.  Network weights are NOT part of it.
//
// The tree pool is packed, not dumped: the pool is provisioned for the population and mostly empty, so only the
// chunks a live tree owns (GameCtl::cur's chunk-id list, n_chunks entries) and the games' spare chunks are copied, each to its
// place in a dense list; restore scatters every chunk back to THE CHUNK ID IT HAD.  Node and block references are global slot
// indices, so nothing is relocated and no search kernel knows a restore happened.  Free chunks and the idle chunk-id list carry
// no meaning and are not saved.  The game record is packed the same way: the moves[g] plies a game has played, not hist_T.
//
// Layout (DESIGN.md 3 "Snapshot"): SnapHdr | host-readable tables (GameCtl, PoolCtl, ring, dense chunk-id list, counters, moves,
// finished games) | RNG streams | packed chunks | packed record.  Sections start on 16-byte boundaries.  tg_sp_restore reads
// the header and the tables on the host and validates them BEFORE anything in the context is overwritten.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "engine.h"
#include "tree_dev.h"

using namespace tg;

namespace {

constexpr char kMagic[8] = {'T', 'G', 'S', 'N', 'A', 'P', '\0', '\0'};
constexpr uint32_t kVersion = 1;

enum Sec {
    SEC_CTL = 0, SEC_POOL, SEC_RING, SEC_CHUNK_IDS, SEC_COUNTERS, SEC_MOVES, SEC_FIN,   // host-readable tables
    SEC_RNG, SEC_TREE, SEC_HIST_OBS, SEC_HIST_CNT, SEC_HIST_PL, SEC_N
};
const char* const kSecName[SEC_N] = {"game_ctl", "pool_ctl", "ring", "chunk_ids", "counters", "moves", "finished",
                                     "rng", "tree", "hist_obs", "hist_cnt", "hist_pl"};

struct SnapSec { uint64_t off, bytes; };
struct SnapHdr {                     // mirrored by transgo_amd/snapshot.py:SnapHdr
    char magic[8];
    uint32_t version, header_bytes;
    // echo of the geometry the data depends on: tg_sp_restore refuses a context that differs in any of these
    int32_t board_size, encode_dim, n_games, parallel_readouts, chunk_slots, pool_chunks, max_chunks, arena_slots, keep_slots, maxd,
        hist_T, record_games, max_step, wu_loss;
    float komi; int32_t pad0;
    double c_puct1, c_puct2;
    // host-side engine state
    int32_t all_reset, n_errors, fin_positions, n_fin;
    uint64_t tree_chunks;            // chunks in the tree section = entries of the dense chunk-id list
    uint64_t hist_plies;             // plies in the record sections
    uint64_t tables_bytes;           // header + host-readable tables = offset of the RNG section
    uint64_t total_bytes;
    SnapSec sec[SEC_N];
};
static_assert(sizeof(SnapHdr) == 336 && sizeof(SnapHdr) % 16 == 0, "fixed header; sections start on 16-byte boundaries");
static_assert(sizeof(GameCtl) == 112 && sizeof(PoolCtl) == 40 && sizeof(tg_mt19937) == 2500, "record sizes are part of the format (version 1)");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// inclusive scan of one int per thread over a 1024-thread workgroup
__device__ __forceinline__ int block_scan_1024(int* part, int v) {
    const int tid = threadIdx.x;
    part[tid] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int t = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    const int r = part[tid];
    __syncthreads();
    return r;
}

// Scan: chunk_off[g] = first entry of game g in the dense chunk list (its live list's n_chunks chunks, then its spare),
// ply_off[g] = first ply of game g in the packed record; entry G of both = the totals; tot = {chunks, plies, games searching}.
__global__ __launch_bounds__(1024) void k_snap_scan(EngineDev d, int32_t* chunk_off, int32_t* ply_off, int32_t* tot) {
    __shared__ int part[1024];
    __shared__ int searching_s;
    const int tid = threadIdx.x, G = d.G;
    const int per = (G + 1023) / 1024, lo = tid * per, hi = lo + per < G ? lo + per : G;
    if (tid == 0) searching_s = 0;
    int nc = 0, np = 0, ns = 0;
    for (int g = lo; g < hi; ++g) {
        const GameCtl* c = &d.ctl[g];
        nc += clampi(c->n_chunks, 0, d.sc.max_chunks) + (c->spare >= 0 ? 1 : 0);
        if (d.hist_obs) np += clampi(c->moves, 0, d.hist_T);
        ns += c->searching ? 1 : 0;
    }
    const int ic = block_scan_1024(part, nc), ip = block_scan_1024(part, np);
    if (ns) atomicAdd(&searching_s, ns);
    int bc = ic - nc, bp = ip - np;
    for (int g = lo; g < hi; ++g) {
        const GameCtl* c = &d.ctl[g];
        chunk_off[g] = bc; ply_off[g] = bp;
        bc += clampi(c->n_chunks, 0, d.sc.max_chunks) + (c->spare >= 0 ? 1 : 0);
        if (d.hist_obs) bp += clampi(c->moves, 0, d.hist_T);
    }
    __syncthreads();
    if (tid == 1023) { chunk_off[G] = ic; ply_off[G] = ip; tot[0] = ic; tot[1] = ip; tot[2] = searching_s; }
}

// One wave per game.  Snapshot: the game's live chunk-id list and its spare go to the dense list.  Restore: the live list is
// written back from it (GameCtl, restored before, says which of the two lists is live and whether the last entry is the spare).
template <bool RESTORE>
__global__ __launch_bounds__(64) void k_snap_list(EngineDev d, const int32_t* chunk_off, int32_t* dense) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const GameCtl* c = &d.ctl[g];
    const int n = clampi(c->n_chunks, 0, d.sc.max_chunks), off = chunk_off[g];
    int32_t* ids = d.chunk_ids + ((size_t)g * 2 + (c->cur & 1)) * (size_t)d.sc.max_chunks;
    for (int i = lane; i < n; i += 64) {
        if (RESTORE) ids[i] = dense[off + i]; else dense[off + i] = ids[i];
    }
    if (!RESTORE && lane == 0 && c->spare >= 0) dense[off + n] = c->spare;
}

// One workgroup per chunk in use: chunk dense[b] of the pool <-> chunk b of the packed tree section, as 16-byte vectors
// (consecutive lanes, consecutive addresses).  A chunk id outside the pool is skipped (restore validates the list on the host).
template <bool RESTORE>
__global__ __launch_bounds__(256) void k_snap_chunks(EngineDev d, const int32_t* dense, uint4* packed) {
    const int id = dense[blockIdx.x];
    if (id < 0 || id >= d.sc.pool_chunks) return;
    const int n4 = d.sc.chunk_slots * (int)(sizeof(NodeRec) / sizeof(uint4));
    uint4* a = reinterpret_cast<uint4*>(d.arena + (size_t)id * d.sc.chunk_slots);
    uint4* p = packed + (size_t)blockIdx.x * n4;
    for (int i = threadIdx.x; i < n4; i += 256) {
        if (RESTORE) a[i] = p[i]; else p[i] = a[i];
    }
}

// One workgroup per game: the plies it has played, hist_* <-> the packed record (a game's plies are contiguous on both sides).
// Unlike the chunks this copy moves 4-byte words (and the side-to-move bytes one by one), not 16-byte vectors: a game's record
// starts at g * hist_T * obs_words words in HBM and at ply_off[g] * obs_words words in the snapshot (26 words per ply at 9x9 with 10
// planes, A = 82 counts), so neither side is 16-byte aligned in general and the two are not aligned to each other.  Consecutive
// lanes still touch consecutive words; the record is a tenth of the trees' bytes (34 MiB against 326 at the headline shape).
template <bool RESTORE>
__global__ __launch_bounds__(256) void k_snap_hist(EngineDev d, const int32_t* ply_off, uint32_t* p_obs, int32_t* p_cnt, uint8_t* p_pl) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const int base = ply_off[g], n = ply_off[g + 1] - base, W = d.obs_words, A = d.sc.A;
    uint32_t* h_obs = d.hist_obs + (size_t)g * d.hist_T * W; uint32_t* s_obs = p_obs + (size_t)base * W;
    int32_t* h_cnt = d.hist_cnt + (size_t)g * d.hist_T * A; int32_t* s_cnt = p_cnt + (size_t)base * A;
    uint8_t* h_pl = d.hist_pl + (size_t)g * d.hist_T; uint8_t* s_pl = p_pl + base;
    for (int i = tid; i < n * W; i += 256) { if (RESTORE) h_obs[i] = s_obs[i]; else s_obs[i] = h_obs[i]; }
    for (int i = tid; i < n * A; i += 256) { if (RESTORE) h_cnt[i] = s_cnt[i]; else s_cnt[i] = h_cnt[i]; }
    for (int i = tid; i < n; i += 256) { if (RESTORE) h_pl[i] = s_pl[i]; else s_pl[i] = h_pl[i]; }
}

uint64_t align16(uint64_t v) { return (v + 15) & ~15ull; }

// The geometry echo of this context.
void fill_echo(const tg_ctx* ctx, SnapHdr* h) {
    const Engine* e = ctx->eng;
    const SearchCfg& sc = e->dev.sc;
    const tg_config& cfg = ctx->cfg;
    h->board_size = ctx->S; h->encode_dim = cfg.encode_dim; h->n_games = e->G; h->parallel_readouts = sc.R;
    h->chunk_slots = sc.chunk_slots; h->pool_chunks = sc.pool_chunks; h->max_chunks = sc.max_chunks; h->arena_slots = sc.arena_slots;
    h->keep_slots = sc.keep_slots; h->maxd = sc.maxd; h->hist_T = e->dev.hist_T; h->record_games = e->dev.hist_obs ? 1 : 0;
    h->max_step = cfg.max_step; h->wu_loss = sc.wu; h->komi = cfg.komi; h->pad0 = 0; h->c_puct1 = sc.c1; h->c_puct2 = sc.c2;
}

// Section table for the given counts (geometry from the header's echo).
void fill_layout(SnapHdr* h, int obs_words, int A) {
    const uint64_t G = (uint64_t)h->n_games;
    uint64_t bytes[SEC_N];
    bytes[SEC_CTL] = sizeof(GameCtl) * G;
    bytes[SEC_POOL] = sizeof(PoolCtl);
    bytes[SEC_RING] = sizeof(int32_t) * (uint64_t)h->pool_chunks;
    bytes[SEC_CHUNK_IDS] = sizeof(int32_t) * h->tree_chunks;
    bytes[SEC_COUNTERS] = sizeof(int32_t) * CNT_N;
    bytes[SEC_MOVES] = sizeof(int32_t) * G;
    bytes[SEC_FIN] = sizeof(int32_t) * 2 * (uint64_t)h->n_fin;
    bytes[SEC_RNG] = sizeof(tg_mt19937) * G;
    bytes[SEC_TREE] = h->tree_chunks * (uint64_t)h->chunk_slots * sizeof(NodeRec);
    bytes[SEC_HIST_OBS] = sizeof(uint32_t) * h->hist_plies * (uint64_t)obs_words;
    bytes[SEC_HIST_CNT] = sizeof(int32_t) * h->hist_plies * (uint64_t)A;
    bytes[SEC_HIST_PL] = h->hist_plies;
    uint64_t off = sizeof(SnapHdr);
    for (int s = 0; s < SEC_N; ++s) {
        if (s == SEC_RNG) h->tables_bytes = off;
        h->sec[s].off = off; h->sec[s].bytes = bytes[s];
        off = align16(off + bytes[s]);
    }
    h->total_bytes = off;
}

#define NEED_ENGINE(ctx) do { if (!(ctx) || !(ctx)->eng || (ctx)->eng->G <= 0) return TG_ERR_ARG; TG_HIP(ctx, hipSetDevice((ctx)->cfg.device)); } while (0)

// offsets of the scan's outputs in Engine::snap_tab: chunk_off i32[G+1] | ply_off i32[G+1] | tot i32[4]
int run_scan(tg_ctx* ctx, int32_t** chunk_off, int32_t** ply_off, int32_t tot[3]) {
    Engine* e = ctx->eng;
    const size_t G1 = (size_t)e->G + 1;
    if (e->snap_tab.reserve(sizeof(int32_t) * (2 * G1 + 4))) TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed");
    *chunk_off = (int32_t*)e->snap_tab.p; *ply_off = *chunk_off + G1;
    int32_t* d_tot = *ply_off + G1;
    hipLaunchKernelGGL(k_snap_scan, dim3(1), dim3(1024), 0, ctx->stream, e->dev, *chunk_off, *ply_off, d_tot);
    TG_HIP(ctx, hipGetLastError());
    TG_HIP(ctx, hipMemcpyAsync(tot, d_tot, sizeof(int32_t) * 3, hipMemcpyDeviceToHost, ctx->stream));
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TG_OK;
}

// Move-boundary check + the header of the snapshot the context would write now.
int prepare(tg_ctx* ctx, const char* who, SnapHdr* h, int32_t** chunk_off, int32_t** ply_off) {
    Engine* e = ctx->eng;
    if (e->batch_kind != BATCH_NONE)
        TG_FAIL(ctx, TG_ERR_STATE, std::string(who) + ": a snapshot is legal at a move boundary only (an evaluation batch is pending)");
    int32_t tot[3];
    int rc = run_scan(ctx, chunk_off, ply_off, tot);
    if (rc) return rc;
    if (tot[2] > 0)
        TG_FAIL(ctx, TG_ERR_STATE, std::string(who) + ": a snapshot is legal at a move boundary only (" + std::to_string(tot[2]) +
                                       " games are inside a search: tg_sp_play has not been called for this move)");
    memset(h, 0, sizeof(*h));
    memcpy(h->magic, kMagic, 8);
    h->version = kVersion; h->header_bytes = (uint32_t)sizeof(SnapHdr);
    fill_echo(ctx, h);
    h->all_reset = e->all_reset ? 1 : 0; h->n_errors = e->n_errors; h->fin_positions = e->fin_positions; h->n_fin = (int32_t)e->fin_slot.size();
    h->tree_chunks = (uint64_t)tot[0]; h->hist_plies = (uint64_t)tot[1];
    fill_layout(h, e->dev.obs_words, ctx->A);
    return TG_OK;
}

std::string mismatch(const char* field, double snap, double mine) {
    char msg[200];
    snprintf(msg, sizeof(msg), "tg_sp_restore: the snapshot was taken with %s = %.9g, this context has %.9g", field, snap, mine);
    return msg;
}

// Everything tg_sp_restore can check on the host: the tables of a snapshot whose header passed.  tab = the first tables_bytes.
// pl = the side-to-move section (one byte per recorded ply, games in slot order), which says how many positions a finished game
// contributes: its plies without the kPlySkip mark.
int validate_tables(tg_ctx* ctx, const SnapHdr& h, const uint8_t* tab, const uint8_t* pl) {
    const SearchCfg& sc = ctx->eng->dev.sc;
    const int G = h.n_games;
    const GameCtl* ctl = (const GameCtl*)(tab + h.sec[SEC_CTL].off);
    const PoolCtl* pc = (const PoolCtl*)(tab + h.sec[SEC_POOL].off);
    const int32_t* ring = (const int32_t*)(tab + h.sec[SEC_RING].off);
    const int32_t* ids = (const int32_t*)(tab + h.sec[SEC_CHUNK_IDS].off);
    const int32_t* moves = (const int32_t*)(tab + h.sec[SEC_MOVES].off);
    const int32_t* fin = (const int32_t*)(tab + h.sec[SEC_FIN].off);
    char msg[200];
    std::vector<uint8_t> seen((size_t)sc.pool_chunks, 0);
    uint64_t at = 0, plies = 0;
    std::vector<uint64_t> ply_at((size_t)G + 1, 0);                    // where game g's plies start in the record sections
    for (int g = 0; g < G; ++g) {
        const GameCtl& c = ctl[g];
        ply_at[g] = plies;
        if (c.cur < 0 || c.cur > 1 || c.n_chunks < 0 || c.n_chunks > sc.max_chunks || c.spare < -1 || c.spare >= sc.pool_chunks || c.root < 0 ||
            c.root >= sc.pool_slots || c.free_slot < 0 || c.free_slot > sc.pool_slots || c.moves < 0 || c.searching) {
            snprintf(msg, sizeof(msg), "tg_sp_restore: the control record of game %d is damaged", g);
            TG_FAIL(ctx, TG_ERR_ARG, msg);
        }
        const uint64_t n = (uint64_t)c.n_chunks + (c.spare >= 0 ? 1 : 0);
        if (at + n > h.tree_chunks) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: the games own more chunks than the snapshot's chunk list holds");
        for (uint64_t i = 0; i < n; ++i) {
            const int32_t id = ids[at + i];
            if (id < 0 || id >= sc.pool_chunks) {
                snprintf(msg, sizeof(msg), "tg_sp_restore: chunk id %d (game %d) is outside the pool of %d chunks", id, g, sc.pool_chunks);
                TG_FAIL(ctx, TG_ERR_ARG, msg);
            }
            if (seen[id]) {
                snprintf(msg, sizeof(msg), "tg_sp_restore: chunk id %d is listed twice (game %d)", id, g);
                TG_FAIL(ctx, TG_ERR_ARG, msg);
            }
            seen[id] = 1;
        }
        if (c.spare >= 0 && ids[at + n - 1] != c.spare) {
            snprintf(msg, sizeof(msg), "tg_sp_restore: game %d's spare chunk is not the one its chunk list names", g);
            TG_FAIL(ctx, TG_ERR_ARG, msg);
        }
        at += n;
        if (h.record_games) plies += (uint64_t)(c.moves < h.hist_T ? c.moves : h.hist_T);
        if (moves[g] < 0) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: negative move count");
    }
    if (at != h.tree_chunks) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: the snapshot's chunk list is longer than what the games own");
    if (plies != h.hist_plies) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: the record sections do not hold the plies the games have played");
    // the free ring: what is poppable must be real chunks, each once, and none of them owned by a tree
    const unsigned long long head = pc->head < pc->visible ? pc->head : pc->visible;
    if (pc->visible > pc->tail || pc->tail - head > (unsigned long long)sc.pool_chunks)
        TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: the pool's ring counters are inconsistent");
    for (unsigned long long k = head; k < pc->tail; ++k) {
        const int32_t id = ring[k % (unsigned long long)sc.pool_chunks];
        if (id < 0 || id >= sc.pool_chunks || seen[id]) {
            snprintf(msg, sizeof(msg), "tg_sp_restore: free-ring entry %d is outside the pool, listed twice or owned by a tree", id);
            TG_FAIL(ctx, TG_ERR_ARG, msg);
        }
        seen[id] = 1;
    }
    int pos = 0;
    for (int i = 0; i < h.n_fin; ++i) {
        const int slot = fin[i], off = fin[h.n_fin + i];
        if (slot < 0 || slot >= G || (i > 0 && slot <= fin[i - 1]) || off != pos)
            TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: the table of finished games is damaged");
        const int n = ctl[slot].moves < h.hist_T ? ctl[slot].moves : h.hist_T;
        if (h.record_games && pl) { for (int t = 0; t < n; ++t) pos += (pl[ply_at[slot] + t] & kPlySkip) ? 0 : 1; }
        else if (h.record_games) pos += n;
    }
    if (pos != h.fin_positions) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: the table of finished games is damaged");
    return TG_OK;
}

}  // namespace

extern "C" {

int tg_sp_snapshot_size(tg_ctx* ctx, uint64_t* bytes) {
    NEED_ENGINE(ctx);
    if (!bytes) return TG_ERR_ARG;
    SnapHdr h; int32_t *coff, *poff;
    int rc = prepare(ctx, "tg_sp_snapshot_size", &h, &coff, &poff);
    if (rc) return rc;
    *bytes = h.total_bytes;
    return TG_OK;
}

int tg_sp_snapshot(tg_ctx* ctx, void* out, uint64_t cap, int device_mem, uint64_t* written) {
    NEED_ENGINE(ctx);
    if (!out) return TG_ERR_ARG;
    Engine* e = ctx->eng;
    const EngineDev& d = e->dev;
    SnapHdr h; int32_t *coff, *poff;
    int rc = prepare(ctx, "tg_sp_snapshot", &h, &coff, &poff);
    if (rc) return rc;
    if (cap < h.total_bytes) {
        char msg[160];
        snprintf(msg, sizeof(msg), "tg_sp_snapshot: the buffer holds %llu bytes, the snapshot needs %llu (tg_sp_snapshot_size)",
                 (unsigned long long)cap, (unsigned long long)h.total_bytes);
        TG_FAIL(ctx, TG_ERR_ARG, msg);
    }
    if (device_mem && ((uintptr_t)out & 15)) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_snapshot: a device buffer must be 16-byte aligned");
    uint8_t* dst = (uint8_t*)out;
    if (!device_mem) {                                                // packed on the device, then ONE copy to the host.  The staging
        // buffer (snapshot-sized, grow-only) stays with the context for the next checkpoint; tg_destroy frees it
        if (e->snap_stage.reserve(h.total_bytes)) TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed (snapshot staging)");
        dst = (uint8_t*)e->snap_stage.p;
    }
    hipStream_t st = ctx->stream;
    for (int s = 0; s < SEC_N; ++s) {                                  // the alignment padding behind a section is zero: a snapshot is compared as bytes
        const uint64_t end = h.sec[s].off + h.sec[s].bytes, pad = align16(end) - end;
        if (pad) TG_HIP(ctx, hipMemsetAsync(dst + end, 0, pad, st));
    }
    auto sec = [&](int s) { return dst + h.sec[s].off; };
    TG_HIP(ctx, hipMemcpyAsync(dst, &h, sizeof(h), hipMemcpyHostToDevice, st));
    TG_HIP(ctx, hipMemcpyAsync(sec(SEC_CTL), d.ctl, h.sec[SEC_CTL].bytes, hipMemcpyDeviceToDevice, st));
    TG_HIP(ctx, hipMemcpyAsync(sec(SEC_POOL), d.pool, h.sec[SEC_POOL].bytes, hipMemcpyDeviceToDevice, st));
    TG_HIP(ctx, hipMemcpyAsync(sec(SEC_RING), d.ring, h.sec[SEC_RING].bytes, hipMemcpyDeviceToDevice, st));
    TG_HIP(ctx, hipMemcpyAsync(sec(SEC_COUNTERS), d.counters, h.sec[SEC_COUNTERS].bytes, hipMemcpyDeviceToDevice, st));
    TG_HIP(ctx, hipMemcpyAsync(sec(SEC_MOVES), e->h_moves.data(), h.sec[SEC_MOVES].bytes, hipMemcpyHostToDevice, st));
    if (h.n_fin) {
        TG_HIP(ctx, hipMemcpyAsync(sec(SEC_FIN), e->fin_slot.data(), sizeof(int32_t) * h.n_fin, hipMemcpyHostToDevice, st));
        TG_HIP(ctx, hipMemcpyAsync(sec(SEC_FIN) + sizeof(int32_t) * h.n_fin, e->fin_off.data(), sizeof(int32_t) * h.n_fin, hipMemcpyHostToDevice, st));
    }
    // the RNG streams in ONE place: the pinned host mirror is the authoritative copy between a search and the next begin_move
    if (e->rng_on_host) TG_HIP(ctx, hipMemcpyAsync(sec(SEC_RNG), e->h_rng, h.sec[SEC_RNG].bytes, hipMemcpyHostToDevice, st));
    else TG_HIP(ctx, hipMemcpyAsync(sec(SEC_RNG), d.rng, h.sec[SEC_RNG].bytes, hipMemcpyDeviceToDevice, st));
    int32_t* dense = (int32_t*)sec(SEC_CHUNK_IDS);
    hipLaunchKernelGGL(k_snap_list<false>, dim3(e->G), dim3(64), 0, st, d, (const int32_t*)coff, dense);
    if (h.tree_chunks)
        hipLaunchKernelGGL(k_snap_chunks<false>, dim3((unsigned)h.tree_chunks), dim3(256), 0, st, d, (const int32_t*)dense, (uint4*)sec(SEC_TREE));
    if (h.hist_plies)
        hipLaunchKernelGGL(k_snap_hist<false>, dim3(e->G), dim3(256), 0, st, d, (const int32_t*)poff, (uint32_t*)sec(SEC_HIST_OBS),
                           (int32_t*)sec(SEC_HIST_CNT), (uint8_t*)sec(SEC_HIST_PL));
    TG_HIP(ctx, hipGetLastError());
    if (!device_mem) TG_HIP(ctx, hipMemcpyAsync(out, dst, h.total_bytes, hipMemcpyDeviceToHost, st));
    TG_HIP(ctx, hipStreamSynchronize(st));
    if (written) *written = h.total_bytes;
    return TG_OK;
}

int tg_sp_restore(tg_ctx* ctx, const void* in, uint64_t bytes, int device_mem) {
    NEED_ENGINE(ctx);
    if (!in) return TG_ERR_ARG;
    Engine* e = ctx->eng;
    EngineDev& d = e->dev;
    hipStream_t st = ctx->stream;
    char msg[200];
    // ---- 1. the header --------------------------------------------------------------------------------------------------------
    if (bytes < sizeof(SnapHdr)) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: truncated snapshot (shorter than its header)");
    if (device_mem && ((uintptr_t)in & 15)) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: a device buffer must be 16-byte aligned");
    SnapHdr h;
    if (device_mem) { TG_HIP(ctx, hipMemcpyAsync(&h, in, sizeof(h), hipMemcpyDeviceToHost, st)); TG_HIP(ctx, hipStreamSynchronize(st)); }
    else memcpy(&h, in, sizeof(h));
    if (memcmp(h.magic, kMagic, 8) != 0) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: not an engine snapshot (wrong magic)");
    if (h.version != kVersion || h.header_bytes != sizeof(SnapHdr)) {
        snprintf(msg, sizeof(msg), "tg_sp_restore: snapshot format version %u (header %u bytes), this library reads version %u (%zu bytes)",
                 h.version, h.header_bytes, kVersion, sizeof(SnapHdr));
        TG_FAIL(ctx, TG_ERR_ARG, msg);
    }
    SnapHdr mine;
    memset(&mine, 0, sizeof(mine));
    fill_echo(ctx, &mine);
#define TG_ECHO(f) do { if (h.f != mine.f) TG_FAIL(ctx, TG_ERR_ARG, mismatch(#f, (double)h.f, (double)mine.f)); } while (0)
    TG_ECHO(board_size); TG_ECHO(encode_dim); TG_ECHO(n_games); TG_ECHO(parallel_readouts); TG_ECHO(record_games); TG_ECHO(max_step);
    TG_ECHO(hist_T); TG_ECHO(chunk_slots); TG_ECHO(pool_chunks); TG_ECHO(arena_slots); TG_ECHO(max_chunks); TG_ECHO(keep_slots); TG_ECHO(maxd);
    TG_ECHO(komi); TG_ECHO(wu_loss); TG_ECHO(c_puct1); TG_ECHO(c_puct2);
#undef TG_ECHO
    for (int s = 0; s < SEC_N; ++s)
        if (h.sec[s].off > bytes || h.sec[s].bytes > bytes - h.sec[s].off) {
            snprintf(msg, sizeof(msg), "tg_sp_restore: truncated snapshot (section %s ends at byte %llu, the buffer holds %llu)", kSecName[s],
                     (unsigned long long)(h.sec[s].off + h.sec[s].bytes), (unsigned long long)bytes);
            TG_FAIL(ctx, TG_ERR_ARG, msg);
        }
    if (h.tree_chunks > (uint64_t)d.sc.pool_chunks || h.hist_plies > (uint64_t)e->G * (uint64_t)(d.hist_T > 0 ? d.hist_T : 0) || h.n_fin < 0 ||
        h.n_fin > e->G || h.fin_positions < 0)
        TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: the header's counts do not fit this context");
    SnapHdr want = h;
    fill_layout(&want, d.obs_words, ctx->A);
    if (memcmp(want.sec, h.sec, sizeof(h.sec)) != 0 || want.tables_bytes != h.tables_bytes || want.total_bytes != h.total_bytes)
        TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: the section table does not match the header's counts");
    if (h.total_bytes > bytes) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_restore: truncated snapshot");
    // ---- 2. the host-readable tables ---------------------------------------------------------------------------------------------
    std::vector<uint8_t> tab_copy;
    const uint8_t* tab = (const uint8_t*)in;
    if (device_mem) {
        tab_copy.resize(h.tables_bytes);
        TG_HIP(ctx, hipMemcpyAsync(tab_copy.data(), in, h.tables_bytes, hipMemcpyDeviceToHost, st));
        TG_HIP(ctx, hipStreamSynchronize(st));
        tab = tab_copy.data();
    }
    // the finished games' position counts depend on their plies' marks: that section is read too (a byte per ply, and only when
    // finished games wait in the snapshot)
    std::vector<uint8_t> pl_copy;
    const uint8_t* pl = nullptr;
    if (h.n_fin > 0 && h.hist_plies) {
        pl = (const uint8_t*)in + h.sec[SEC_HIST_PL].off;
        if (device_mem) {
            pl_copy.resize(h.sec[SEC_HIST_PL].bytes);
            TG_HIP(ctx, hipMemcpyAsync(pl_copy.data(), pl, pl_copy.size(), hipMemcpyDeviceToHost, st));
            TG_HIP(ctx, hipStreamSynchronize(st));
            pl = pl_copy.data();
        }
    }
    int rc = validate_tables(ctx, h, tab, pl);
    if (rc) return rc;
    // staging and scratch are allocated while a failure still leaves the context as it was
    const uint8_t* src = (const uint8_t*)in;
    if (!device_mem) {
        if (e->snap_stage.reserve(h.total_bytes)) TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed (snapshot staging)");
        src = (const uint8_t*)e->snap_stage.p;
    }
    if (e->snap_tab.reserve(sizeof(int32_t) * (2 * ((size_t)e->G + 1) + 4))) TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed");
    // ---- 3. commit --------------------------------------------------------------------------------------------------------------
    if (!device_mem) TG_HIP(ctx, hipMemcpyAsync(e->snap_stage.p, in, h.total_bytes, hipMemcpyHostToDevice, st));
    auto sec = [&](int s) { return src + h.sec[s].off; };
    TG_HIP(ctx, hipMemcpyAsync(d.ctl, sec(SEC_CTL), h.sec[SEC_CTL].bytes, hipMemcpyDeviceToDevice, st));
    TG_HIP(ctx, hipMemcpyAsync(d.pool, sec(SEC_POOL), h.sec[SEC_POOL].bytes, hipMemcpyDeviceToDevice, st));
    TG_HIP(ctx, hipMemcpyAsync(d.ring, sec(SEC_RING), h.sec[SEC_RING].bytes, hipMemcpyDeviceToDevice, st));
    TG_HIP(ctx, hipMemcpyAsync(d.counters, sec(SEC_COUNTERS), h.sec[SEC_COUNTERS].bytes, hipMemcpyDeviceToDevice, st));
    TG_HIP(ctx, hipMemcpyAsync(d.rng, sec(SEC_RNG), h.sec[SEC_RNG].bytes, hipMemcpyDeviceToDevice, st));
    TG_HIP(ctx, hipMemsetAsync(d.ply_skip, 0, (size_t)e->G, st));      // a snapshot is a move boundary: no record switch is in flight
    TG_HIP(ctx, hipMemsetAsync(e->d_forced, 0, (size_t)e->G, st));     // ... and no forced move (a snapshot inside a move's search is refused)
    TG_HIP(ctx, hipMemsetAsync(e->d_gumbel, 0, (size_t)e->G, st));     // ... nor a Gumbel move
    { int rc2 = own_clear(ctx, nullptr); if (rc2) return rc2; }        // search ownership is per search and not part of a snapshot
    int32_t *coff, *poff; int32_t tot[3];
    rc = run_scan(ctx, &coff, &poff, tot);                             // the offsets, from the control records just restored
    if (rc) return rc;
    hipLaunchKernelGGL(k_snap_list<true>, dim3(e->G), dim3(64), 0, st, d, (const int32_t*)coff, (int32_t*)sec(SEC_CHUNK_IDS));
    if (h.tree_chunks)
        hipLaunchKernelGGL(k_snap_chunks<true>, dim3((unsigned)h.tree_chunks), dim3(256), 0, st, d, (const int32_t*)sec(SEC_CHUNK_IDS), (uint4*)sec(SEC_TREE));
    if (h.hist_plies)
        hipLaunchKernelGGL(k_snap_hist<true>, dim3(e->G), dim3(256), 0, st, d, (const int32_t*)poff, (uint32_t*)sec(SEC_HIST_OBS),
                           (int32_t*)sec(SEC_HIST_CNT), (uint8_t*)sec(SEC_HIST_PL));
    TG_HIP(ctx, hipGetLastError());
    const int32_t* moves = (const int32_t*)(tab + h.sec[SEC_MOVES].off);
    const int32_t* fin = (const int32_t*)(tab + h.sec[SEC_FIN].off);
    e->h_moves.assign(moves, moves + e->G);
    e->fin_slot.assign(fin, fin + h.n_fin); e->fin_off.assign(fin + h.n_fin, fin + 2 * h.n_fin); e->fin_positions = h.fin_positions; ++e->fin_seq;
    e->all_reset = h.all_reset != 0; e->n_errors = h.n_errors;
    e->batch_kind = BATCH_NONE; e->batch_ready = false; e->last_rows = 0;
    e->rng_on_host = false;                                            // the device copy is the one just written
    TG_HIP(ctx, hipStreamSynchronize(st));
    return TG_OK;
}

}  // extern "C"
