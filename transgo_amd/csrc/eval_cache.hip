// eval_cache.hip -- exact evaluation cache around the network forward of the self-play engine (tg_sp_eval_cache).
//
// The network's output for a row is a pure function of the row's bit-packed planes (EngineDev::obs_bits), the live weight set and
// the symmetry mode, and the forward gives identical bits for identical rows wherever they stand in the batch.  So a table keyed
// by the FULL bits (the hash only picks the bucket) can hand back policy / value instead of evaluating: no float in the tree
// changes, only rows leave the forward.  A pending batch of `rows` rows runs as
//   k_ec_probe    one wave per row: hash, bucket, way = tag + generation + every word equal -> policy[row] / value[row] from the
//                 entry; a miss elects the lowest row of its hash in a per-batch scratch set (atomicMin)
//   k_ec_resolve  one wave per missed row: a row whose elected representative is another row follows it only if all words match
//   k_ec_compact  one workgroup: the rows that evaluate themselves, in row order -> dense slot list, its length M, the counters
//   (host reads M; the unchanged forward runs on those M rows into staging buffers; M == 0 launches nothing)
//   k_ec_finish   one wave per missed row: policy / value from its representative's staging row; evaluated rows insert themselves:
//                 a way is claimed by ONE atomicCAS on the header's claim word (the batch's sequence number), only the claimant
//                 writes, a loser drops its insert.  Readers run in the next batch's k_ec_probe, never beside a writer.
//   k_ec_tally    one workgroup: insert / drop counts of the batch
// Invalidation is the generation number in the header (eval_cache_invalidate): nothing is swept.
#include <string>

#include "engine.h"

namespace tg {

constexpr int kEcWays = 4;
constexpr int kEcLaneWords = 3;                   // words a lane holds: rows of up to 192 words (13 planes of 19x19 are 147)
enum { EC_LOOKUPS = 0, EC_HITS, EC_DUPS, EC_EVALUATED, EC_INSERTS, EC_DROPPED, EC_NSTAT };
enum { EC_CODE_NONE = 0, EC_CODE_INSERTED = 1, EC_CODE_DROPPED = 2 };

// Everything the cache kernels need, passed by value.
struct ECDev {
    uint4* hdr = nullptr;           // [entries] x: claim (sequence number of the batch that last wrote the way), y: generation (0 = never
                                    //           written), z / w: low / high half of the key's hash
    uint32_t* keys = nullptr;       // [entries][W]   the row's words, the unused high bits of the last one masked off
    float* pay = nullptr;           // [entries][A + 1]  policy, then value
    uint32_t n_buckets = 0, gen = 1, seq = 0;
    uint32_t* scratch = nullptr;    // [scratch_mask + 1] per-batch set: lowest missed row of each hash slot (0xffffffff = none)
    uint32_t scratch_mask = 0;
    unsigned long long* hash = nullptr;   // [rows_cap]
    int32_t* rep = nullptr;         // [rows_cap] -1: hit; else the row whose evaluation serves this one (itself = evaluated)
    int32_t* eidx = nullptr;        // [rows_cap] staging row of an evaluated row
    int32_t* eval_slot = nullptr;   // [rows_cap] dense list of the obs_bits slots to evaluate
    uint8_t* code = nullptr;        // [rows_cap] EC_CODE_* of the batch's inserts
    float* st_pol = nullptr;        // [rows_cap][A] staging outputs of the forward
    float* st_val = nullptr;        // [rows_cap]
    unsigned long long* stats = nullptr;   // [EC_NSTAT]
    int32_t* m_out = nullptr;       // length of eval_slot, where the host reads it
    int W = 0, A = 0;
    uint32_t tail_mask = 0xffffffffu;
};

struct EvalCache {
    ECDev d;
    uint64_t entries = 0, bytes = 0;
    // HIP-event timing per batch (tg_prof_enable_eval_cache): 5 events = probe..compact | read-back gap | forward | finish + tally
    bool prof = false; std::vector<hipEvent_t> ev; size_t ev_used = 0;
    double probe_ms = 0, readback_ms = 0, net_ms = 0, insert_ms = 0; long batches = 0;
};

}  // namespace tg

namespace {

using namespace tg;

__device__ __forceinline__ uint64_t ec_mix(uint64_t x) {             // splitmix64's finaliser
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}

// The calling wave's row: word i = lane + 64 k in w[k] (0 beyond W), and the row's 64-bit hash -- every word mixed with its own
// position, summed over the wave (order-free), finalised.  Returned in every lane.
__device__ __forceinline__ uint64_t ec_load_row(const ECDev& c, const uint32_t* __restrict__ bits, int slot, int lane,
                                                uint32_t (&w)[kEcLaneWords]) {
    const uint32_t* in = bits + (size_t)slot * c.W;
    uint64_t h = 0;
#pragma unroll
    for (int k = 0; k < kEcLaneWords; ++k) {
        const int i = lane + 64 * k;
        uint32_t v = 0;
        if (i < c.W) {
            v = in[i];
            if (i == c.W - 1) v &= c.tail_mask;
            h += ec_mix((uint64_t)v + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1));
        }
        w[k] = v;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)h, off, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(h >> 32), off, 64);
        h += ((uint64_t)hi << 32) | lo;
    }
    return ec_mix(h);
}

// every word of the wave's row equals the W words at `other` (which are stored or compared masked)
__device__ __forceinline__ bool ec_same(const ECDev& c, const uint32_t* __restrict__ other, bool mask_tail, int lane,
                                        const uint32_t (&w)[kEcLaneWords]) {
    bool eq = true;
#pragma unroll
    for (int k = 0; k < kEcLaneWords; ++k) {
        const int i = lane + 64 * k;
        if (i < c.W) {
            uint32_t v = other[i];
            if (mask_tail && i == c.W - 1) v &= c.tail_mask;
            eq = eq && v == w[k];
        }
    }
    return __all(eq) != 0;
}

__global__ __launch_bounds__(256) void k_ec_probe(ECDev c, const uint32_t* __restrict__ bits, const int32_t* __restrict__ row_slot,
                                                  float* __restrict__ policy, float* __restrict__ value, int rows) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    uint32_t w[kEcLaneWords];
    const uint64_t h = ec_load_row(c, bits, row_slot[row], lane, w);
    const size_t e0 = (size_t)(h % c.n_buckets) * kEcWays;
    const uint32_t tag_lo = (uint32_t)h, tag_hi = (uint32_t)(h >> 32);
    for (int way = 0; way < kEcWays; ++way) {
        const size_t e = e0 + way;
        const uint4 hd = c.hdr[e];                                    // one address per wave
        if (hd.y != c.gen || hd.z != tag_lo || hd.w != tag_hi) continue;
        if (!ec_same(c, c.keys + e * c.W, false, lane, w)) continue;
        const float* p = c.pay + e * (size_t)(c.A + 1);
        for (int j = lane; j < c.A; j += 64) policy[(size_t)row * c.A + j] = p[j];
        if (lane == 0) { value[row] = p[c.A]; c.rep[row] = -1; }
        return;
    }
    if (lane == 0) {
        c.hash[row] = h;
        c.rep[row] = row;
        atomicMin(&c.scratch[(uint32_t)(h >> 20) & c.scratch_mask], (uint32_t)row);
    }
}

__global__ __launch_bounds__(256) void k_ec_resolve(ECDev c, const uint32_t* __restrict__ bits, const int32_t* __restrict__ row_slot, int rows) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    if (c.rep[row] < 0) return;
    const uint64_t h = c.hash[row];
    const uint32_t r0 = c.scratch[(uint32_t)(h >> 20) & c.scratch_mask];
    if (r0 >= (uint32_t)row) return;                                  // this row is the elected one (r0 > row never happens: atomicMin)
    // r0 missed too and owns its scratch slot, so it evaluates itself: following it never chains
    uint32_t w[kEcLaneWords];
    (void)ec_load_row(c, bits, row_slot[row], lane, w);
    if (ec_same(c, bits + (size_t)row_slot[r0] * c.W, true, lane, w) && lane == 0) c.rep[row] = (int32_t)r0;
}

__global__ __launch_bounds__(1024) void k_ec_compact(ECDev c, const int32_t* __restrict__ row_slot, int rows) {
    __shared__ int part[1024];
    __shared__ int hits_s, dups_s;
    const int tid = threadIdx.x;
    const int per = (rows + 1023) / 1024, lo = tid * per < rows ? tid * per : rows, hi = lo + per < rows ? lo + per : rows;
    if (tid == 0) { hits_s = 0; dups_s = 0; }
    int ev = 0, hits = 0, dups = 0;
    for (int r = lo; r < hi; ++r) { const int p = c.rep[r]; ev += p == r; hits += p < 0; dups += p >= 0 && p != r; }
    part[tid] = ev;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {                        // inclusive scan over the 1024 partial sums
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    if (hits) atomicAdd(&hits_s, hits);
    if (dups) atomicAdd(&dups_s, dups);
    int base = part[tid] - ev;
    for (int r = lo; r < hi; ++r)
        if (c.rep[r] == r) { c.eval_slot[base] = row_slot[r]; c.eidx[r] = base; ++base; }
    __syncthreads();
    if (tid == 0) {
        *c.m_out = part[1023];
        c.stats[EC_LOOKUPS] += (unsigned long long)rows; c.stats[EC_HITS] += (unsigned long long)hits_s;
        c.stats[EC_DUPS] += (unsigned long long)dups_s; c.stats[EC_EVALUATED] += (unsigned long long)part[1023];
    }
}

__global__ __launch_bounds__(256) void k_ec_finish(ECDev c, const uint32_t* __restrict__ bits, const int32_t* __restrict__ row_slot,
                                                   float* __restrict__ policy, float* __restrict__ value, int rows) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int r = c.rep[row];
    if (r < 0) { if (lane == 0) c.code[row] = EC_CODE_NONE; return; }
    const size_t m = (size_t)c.eidx[r];
    const float* sp = c.st_pol + m * c.A;
    for (int j = lane; j < c.A; j += 64) policy[(size_t)row * c.A + j] = sp[j];
    const float v = c.st_val[m];
    if (lane == 0) value[row] = v;
    if (r != row) { if (lane == 0) c.code[row] = EC_CODE_NONE; return; }
    // insert: a way nobody wrote in this generation if the bucket has one, else one picked by the hash
    uint32_t w[kEcLaneWords];
    const uint64_t h = ec_load_row(c, bits, row_slot[row], lane, w);
    const size_t e0 = (size_t)(h % c.n_buckets) * kEcWays;
    int claimed = -1, result = EC_CODE_DROPPED;
    for (int pass = 0; pass <= kEcWays && claimed < 0; ++pass) {
        const int way = pass < kEcWays ? pass : (int)((h >> 44) & (kEcWays - 1));
        const uint4 hd = c.hdr[e0 + way];
        if (hd.x == c.seq) continue;                                  // claimed by another row of this batch
        if (pass < kEcWays && hd.y == c.gen) continue;                // live entry: only the last pass overwrites
        int ok = 0;
        if (lane == 0) ok = atomicCAS(reinterpret_cast<unsigned int*>(&c.hdr[e0 + way]), hd.x, c.seq) == hd.x;
        ok = __shfl(ok, 0, 64);
        if (ok) { claimed = way; result = EC_CODE_INSERTED; }
    }
    if (claimed >= 0) {
        const size_t e = e0 + claimed;
#pragma unroll
        for (int k = 0; k < kEcLaneWords; ++k) { const int i = lane + 64 * k; if (i < c.W) c.keys[e * c.W + i] = w[k]; }
        float* p = c.pay + e * (size_t)(c.A + 1);
        for (int j = lane; j < c.A; j += 64) p[j] = sp[j];
        if (lane == 0) {
            p[c.A] = v;
            uint32_t* hw = reinterpret_cast<uint32_t*>(&c.hdr[e]);
            hw[1] = c.gen; hw[2] = (uint32_t)h; hw[3] = (uint32_t)(h >> 32);
        }
    }
    if (lane == 0) c.code[row] = (uint8_t)result;
}

__global__ __launch_bounds__(1024) void k_ec_tally(ECDev c, int rows) {
    __shared__ int ins_s, drop_s;
    const int tid = threadIdx.x;
    if (tid == 0) { ins_s = 0; drop_s = 0; }
    __syncthreads();
    int ins = 0, drop = 0;
    for (int r = tid; r < rows; r += 1024) { const int k = c.code[r]; ins += k == EC_CODE_INSERTED; drop += k == EC_CODE_DROPPED; }
    if (ins) atomicAdd(&ins_s, ins);
    if (drop) atomicAdd(&drop_s, drop);
    __syncthreads();
    if (tid == 0) { c.stats[EC_INSERTS] += (unsigned long long)ins_s; c.stats[EC_DROPPED] += (unsigned long long)drop_s; }
}

void ec_free(EvalCache* c) {
    void* ptrs[] = {c->d.hdr, c->d.keys, c->d.pay, c->d.scratch, c->d.hash, c->d.rep, c->d.eidx, c->d.eval_slot, c->d.code,
                    c->d.st_pol, c->d.st_val, c->d.stats, c->d.m_out};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    for (hipEvent_t ev : c->ev) (void)hipEventDestroy(ev);
    delete c;
}

}  // namespace

namespace tg {

void eval_cache_invalidate(tg_ctx* ctx) {
    if (ctx && ctx->eng && ctx->eng->cache) ctx->eng->cache->d.gen++;
}

void eval_cache_destroy(tg_ctx* ctx) {
    if (!ctx || !ctx->eng || !ctx->eng->cache) return;
    (void)hipStreamSynchronize(ctx->stream);
    ec_free(ctx->eng->cache);
    ctx->eng->cache = nullptr;
}

int eval_cache_run(tg_ctx* ctx, int rows) {
    Engine* e = ctx->eng;
    EvalCache* ec = e->cache;
    if (rows <= 0) return TG_OK;
    if (rows > e->rows_cap) TG_FAIL(ctx, TG_ERR_ARG, "evaluation batch larger than the engine's row capacity");
    if (!e->net) TG_FAIL(ctx, TG_ERR_STATE, "no network weights loaded (tg_net_load)");
    ECDev& c = ec->d;
    c.seq++;
    if (c.seq == 0) c.seq = 1;
    const bool timed = ec->prof && ec->ev_used + 5 <= ec->ev.size();
    hipEvent_t* ev = timed ? &ec->ev[ec->ev_used] : nullptr;
    const int grid = (rows + 3) / 4;
    if (timed) TG_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    TG_HIP(ctx, hipMemsetAsync(c.scratch, 0xff, sizeof(uint32_t) * ((size_t)c.scratch_mask + 1), ctx->stream));
    hipLaunchKernelGGL(k_ec_probe, dim3(grid), dim3(256), 0, ctx->stream, c, (const uint32_t*)e->dev.obs_bits,
                       (const int32_t*)e->dev.row_slot, e->dev.policy, e->dev.value, rows);
    hipLaunchKernelGGL(k_ec_resolve, dim3(grid), dim3(256), 0, ctx->stream, c, (const uint32_t*)e->dev.obs_bits,
                       (const int32_t*)e->dev.row_slot, rows);
    hipLaunchKernelGGL(k_ec_compact, dim3(1), dim3(1024), 0, ctx->stream, c, (const int32_t*)e->dev.row_slot, rows);
    TG_HIP(ctx, hipGetLastError());
    if (timed) TG_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    int32_t M = 0;                                                    // the forward's launch geometry needs it: one small read-back per batch
    TG_HIP(ctx, hipMemcpyAsync(&M, c.m_out, sizeof(M), hipMemcpyDeviceToHost, ctx->stream));
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (M < 0 || M > rows) TG_FAIL(ctx, TG_ERR_STATE, "evaluation cache: bad count of rows to evaluate");
    if (timed) TG_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
    if (M > 0) { int rc = tg_net_forward_rows(ctx, M, c.eval_slot, c.st_pol, c.st_val); if (rc) return rc; }
    if (timed) TG_HIP(ctx, hipEventRecord(ev[3], ctx->stream));
    if (M > 0) {                                                      // every row hit: nothing to scatter or insert
        hipLaunchKernelGGL(k_ec_finish, dim3(grid), dim3(256), 0, ctx->stream, c, (const uint32_t*)e->dev.obs_bits,
                           (const int32_t*)e->dev.row_slot, e->dev.policy, e->dev.value, rows);
        hipLaunchKernelGGL(k_ec_tally, dim3(1), dim3(1024), 0, ctx->stream, c, rows);
        TG_HIP(ctx, hipGetLastError());
    }
    if (timed) { TG_HIP(ctx, hipEventRecord(ev[4], ctx->stream)); ec->ev_used += 5; }
    return TG_OK;
}

}  // namespace tg

extern "C" {

int tg_sp_eval_cache(tg_ctx* ctx, uint64_t entries) {
    if (!ctx) return TG_ERR_ARG;
    if (!ctx->eng || ctx->eng->G <= 0) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_eval_cache: the context has no self-play engine (n_games = 0)");
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    Engine* e = ctx->eng;
    if (e->batch_kind != BATCH_NONE) TG_FAIL(ctx, TG_ERR_STATE, "tg_sp_eval_cache: an evaluation batch is pending");
    if (entries && e->own_on)
        TG_FAIL(ctx, TG_ERR_STATE, "tg_sp_eval_cache: search ownership is on (tg_sp_search_ownership); the cache stores policy and value only, so a hit has no ownership to give");
    const int W = e->dev.obs_words, A = ctx->A;
    if (entries && W > 64 * kEcLaneWords) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_eval_cache: rows of more than 192 words are not supported");
    if (entries > (1ull << 31)) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_eval_cache: at most 2^31 entries");
    eval_cache_destroy(ctx);
    if (entries == 0) return TG_OK;
    const uint64_t buckets = (entries + kEcWays - 1) / kEcWays;
    entries = buckets * kEcWays;
    size_t scratch = 64;
    while (scratch < 2 * (size_t)e->rows_cap) scratch <<= 1;
    const size_t rc = (size_t)e->rows_cap;
    EvalCache* ec = new EvalCache();
    ECDev& c = ec->d;
    struct { void** p; size_t bytes; } want[] = {
        {(void**)&c.hdr, sizeof(uint4) * entries}, {(void**)&c.keys, sizeof(uint32_t) * entries * W},
        {(void**)&c.pay, sizeof(float) * entries * (A + 1)}, {(void**)&c.scratch, sizeof(uint32_t) * scratch},
        {(void**)&c.hash, sizeof(unsigned long long) * rc}, {(void**)&c.rep, sizeof(int32_t) * rc}, {(void**)&c.eidx, sizeof(int32_t) * rc},
        {(void**)&c.eval_slot, sizeof(int32_t) * rc}, {(void**)&c.code, rc}, {(void**)&c.st_pol, sizeof(float) * rc * A},
        {(void**)&c.st_val, sizeof(float) * rc}, {(void**)&c.stats, sizeof(unsigned long long) * EC_NSTAT}, {(void**)&c.m_out, sizeof(int32_t)}};
    size_t total = 0;
    for (auto& w : want) total += w.bytes;
    for (auto& w : want) {
        const hipError_t er = hipMalloc(w.p, w.bytes);
        if (er != hipSuccess) {
            (void)hipGetLastError();
            ec_free(ec);
            TG_FAIL(ctx, TG_ERR_HIP, "tg_sp_eval_cache: hipMalloc failed (" + std::string(hipGetErrorString(er)) + ") for a cache of " +
                                         std::to_string(entries) + " entries: " + std::to_string(total) + " bytes asked for, " +
                                         std::to_string(w.bytes) + " in the allocation that failed");
        }
    }
    c.n_buckets = (uint32_t)buckets; c.gen = 1; c.seq = 0; c.scratch_mask = (uint32_t)(scratch - 1);
    c.W = W; c.A = A;
    const int nbits = ctx->cfg.encode_dim * ctx->P;
    c.tail_mask = (nbits & 31) ? (1u << (nbits & 31)) - 1u : 0xffffffffu;
    ec->entries = entries; ec->bytes = total;
    e->cache = ec;
    TG_HIP(ctx, hipMemsetAsync(c.hdr, 0, sizeof(uint4) * entries, ctx->stream));
    TG_HIP(ctx, hipMemsetAsync(c.stats, 0, sizeof(unsigned long long) * EC_NSTAT, ctx->stream));
    TG_HIP(ctx, hipMemsetAsync(c.code, 0, rc, ctx->stream));
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TG_OK;
}

int tg_sp_eval_cache_clear(tg_ctx* ctx) {
    if (!ctx) return TG_ERR_ARG;
    tg::eval_cache_invalidate(ctx);
    return TG_OK;
}

int tg_sp_eval_cache_stats(tg_ctx* ctx, uint64_t* lookups, uint64_t* hits, uint64_t* batch_duplicates, uint64_t* evaluated,
                           uint64_t* inserts, uint64_t* dropped_inserts, uint64_t* entries, uint64_t* bytes) {
    if (!ctx) return TG_ERR_ARG;
    unsigned long long s[EC_NSTAT] = {0};
    EvalCache* ec = ctx->eng ? ctx->eng->cache : nullptr;
    if (ec) {
        TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
        TG_HIP(ctx, hipMemcpyAsync(s, ec->d.stats, sizeof(s), hipMemcpyDeviceToHost, ctx->stream));
        TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (lookups) *lookups = s[EC_LOOKUPS];
    if (hits) *hits = s[EC_HITS];
    if (batch_duplicates) *batch_duplicates = s[EC_DUPS];
    if (evaluated) *evaluated = s[EC_EVALUATED];
    if (inserts) *inserts = s[EC_INSERTS];
    if (dropped_inserts) *dropped_inserts = s[EC_DROPPED];
    if (entries) *entries = ec ? ec->entries : 0;
    if (bytes) *bytes = ec ? ec->bytes : 0;
    return TG_OK;
}

// HIP-event timing of the cache's stages around the forward, per batch, on the context's stream (as tg_prof_enable_tree does it):
// probe_ms = scratch reset + probe + resolve + compact, readback_ms = the stream's idle gap while the host reads the row count,
// net_ms = the forward on the rows left, insert_ms = scatter-and-insert + tally.
int tg_prof_enable_eval_cache(tg_ctx* ctx, int on, int max_batches) {
    if (!ctx || !ctx->eng || !ctx->eng->cache) return TG_ERR_STATE;
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    EvalCache* ec = ctx->eng->cache;
    if (on) {
        const size_t want = 5 * (size_t)(max_batches > 0 ? max_batches : 1024);
        while (ec->ev.size() < want) { hipEvent_t ev; TG_HIP(ctx, hipEventCreate(&ev)); ec->ev.push_back(ev); }
        ec->ev_used = 0; ec->probe_ms = ec->readback_ms = ec->net_ms = ec->insert_ms = 0; ec->batches = 0;
    }
    ec->prof = on != 0;
    return TG_OK;
}

int tg_prof_read_eval_cache(tg_ctx* ctx, double* probe_ms, double* readback_ms, double* net_ms, double* insert_ms, int64_t* batches) {
    if (!ctx || !ctx->eng || !ctx->eng->cache) return TG_ERR_STATE;
    EvalCache* ec = ctx->eng->cache;
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i + 4 < ec->ev_used; i += 5) {
        double* dst[4] = {&ec->probe_ms, &ec->readback_ms, &ec->net_ms, &ec->insert_ms};
        for (int k = 0; k < 4; ++k) { float t = 0; TG_HIP(ctx, hipEventElapsedTime(&t, ec->ev[i + k], ec->ev[i + k + 1])); *dst[k] += t; }
        ec->batches++;
    }
    ec->ev_used = 0;
    if (probe_ms) *probe_ms = ec->probe_ms;
    if (readback_ms) *readback_ms = ec->readback_ms;
    if (net_ms) *net_ms = ec->net_ms;
    if (insert_ms) *insert_ms = ec->insert_ms;
    if (batches) *batches = ec->batches;
    return TG_OK;
}

}  // extern "C"
