// gwaoi_sync.hip -- entity position sync around the AOI path (include/gwaoi_sync.h).
//
// Five device passes, all on the world's stream:
//   decode    HandleSyncPositionYawFromClient (GameService.go:392-404): one
//             lane per 32-B record, entity-id hash lookup, the record becomes
//             op i of a device Moved batch (SLOT_NONE = skipped), Y/yaw by
//             last-writer claim, sifSyncNeighborClients.
//   fan-out   CollectEntitySyncInfos (Entity.go:1221-1267), receiver side:
//             one lane per frame entity B with a client; its records are its
//             own (sifSyncOwnClient) and one per flagged A with rel(A,B) (the
//             go-aoi relation of the last flush: B in A.InterestedBy).
//   route     Entity.interest/uninterest -> sendCreateEntity/sendDestroyEntity
//             (Entity.go:236-246, GameClient.go:37-59): the flush's events
//             whose first entity has a client, grouped by gate.
//   broadcast Entity.CallAllClients / ForAllClients / send*AttrChange...ToClients
//             (Entity.go:743-917), source side: one wave per (source, flags)
//             message; a record for the source's own client and one per B with
//             rel(source, B) that has a client, grouped by gate.
//   switch    Entity.SetClient / GiveClientTo (Entity.go:678-765), source side: one wave per
//             (slot, new client) message; a destroy record for the old client and a create
//             record for the new one per B with rel(source, B), grouped by gate; then the
//             clients are switched.
// and the interest-set reads of game logic (loops over InterestedIn, Entity.IsInterestedIn,
// Entity.DistanceTo: Monster.go:49-91, Entity.go:248-256), which deliver nothing and change nothing:
//   rows      one wave per query slot over the broadcast's window walk; count pass, scan, write pass.
//   related   one lane per (a, b) pair: two rank lookups, two frame records, one rel().
//   nearest   one wave per query: the neighbour passing a tag filter with the smallest (d2, slot).
// Grouping by gate is a multisplit: a first pass counts records per
// (gate, block) in LDS, an exclusive scan gives every (gate, block) its
// base, a second pass writes each block's runs (the fan-out's first pass
// also lists every record's sender, so the AOI window is walked once).
// The output is HBM write bound (48 B per record).

#include "gwaoi_device.h"
#include "gwaoi_internal.h"
#include "gwaoi_mem.h"
#include "../../include/gwaoi_sync.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace gw {
namespace {

constexpr uint32_t NO_GATE = 0xFFFFFFFFu;
constexpr uint32_t H_EMPTY = 0xFFFFFFFFu;  // hash bucket never used
constexpr uint32_t H_TOMB = 0xFFFFFFFEu;   // hash bucket freed
constexpr int ST = 256;                    // threads per workgroup of the sync kernels
constexpr uint32_t SCR_FULL = 0xFFFFFFFFu; // fan-out: the block's hits did not fit the scratch

inline uint32_t cdivu(size_t a, size_t b) { return (uint32_t)((a + b - 1) / b); }

// Hash of a 16-byte id (host and device agree).
__host__ __device__ inline uint32_t id_hash(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    unsigned long long h = (((unsigned long long)b << 32) | a) * 0x9E3779B97F4A7C15ull;
    h ^= (((unsigned long long)d << 32) | c) + 0x632BE59BD9B4E019ull + (h << 6) + (h >> 2);
    h ^= h >> 31;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
    return (uint32_t)h;
}

// The fan-out's 16-B output and scratch stores.  Plain stores: the non-temporal form was
// slower.
// 16-B record stores that nothing in the kernel reads back: nontemporal (A/B,
// profiles/r06_ab_fan_write.txt: k_fan_write 661 -> 630 us against plain stores)
__device__ __forceinline__ void st_stream(uint4 *p, const uint4 &v) {
#ifdef GWAOI_EXP_FW_PLAIN
    *p = v;
#else
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    const v4u x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<v4u *>(p));
#endif
}

__device__ __forceinline__ bool eq4(uint4 a, uint4 b) {
    return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
}

// ------------------------------------------------------------ scatter ------
// Host-side state changes reach the device as (array, index, value) writes.
constexpr int MAX_ARR = 8;
struct ArrTable {
    void *p[MAX_ARR];
    uint32_t stride[MAX_ARR];  // elements between consecutive indices (fields of packed per-slot records)
};
struct W32 {
    uint32_t arr, idx, val, pad;
};
struct W128 {
    uint32_t arr, idx, pad0, pad1;
    uint4 val;
};

__global__ void k_scatter32(const W32 *__restrict__ w, uint32_t n, ArrTable T) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const W32 e = w[i];
    static_cast<uint32_t *>(T.p[e.arr])[(size_t)e.idx * T.stride[e.arr]] = e.val;
}

__global__ void k_scatter128(const W128 *__restrict__ w, uint32_t n, ArrTable T) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const W128 e = w[i];
    static_cast<uint4 *>(T.p[e.arr])[(size_t)e.idx * T.stride[e.arr]] = e.val;
}

// Per-slot sync state is packed so that one pass touches one line per slot:
//   one 64-B record per slot (SLOT_U4 uint4): sst {gate index, space in call
//           order, syncing, sync flags}, pos {x, y, z, yaw}, eid, cid -- the
//           fan-out's sender pass reads the first three from one line, the
//           decode writes pos and the flags into it
//   cl[s]   ulonglong2 {Position claim, yaw claim}
//   htab    64-B buckets {3 entity ids; their 3 slots}: a probe reads keys and
//           values from one line (see lookup).
enum SstField { SST_GATE = 0, SST_SPACE = 1, SST_SYNCING = 2, SST_FLAGS = 3 };
constexpr uint32_t SLOT_U4 = 4;             // uint4 per slot record: sst, pos, eid, cid
constexpr uint32_t SLOT_W = 4 * SLOT_U4;    // its 32-bit words

// Host position/yaw writes (set_position_yaw, entity_set_position_yaw,
// entity_enter_plain) and flag-only ops (Space.enter): claim, then the winner
// writes.  Position (x, y, z) and yaw have claims of their own: outside an AOI
// space setPositionYaw changes yaw but not Position (Space.go:253-257), so the
// last write of each may come from different calls.
constexpr uint32_t SIDE_POS = 0x100u;  // op writes Position (x, y, z)
constexpr uint32_t SIDE_YAW = 0x200u;  // op writes yaw
constexpr uint32_t SIDE_SIF = GWAOI_SIF_OWN_CLIENT | GWAOI_SIF_NEIGHBOR_CLIENTS;
struct SideOp {
    uint32_t slot, bits;  // bits: SIDE_POS | SIDE_YAW | sync flags
    unsigned long long claim;
    float4 pos;  // x, y, z, yaw
};

__global__ void k_side_claim(const SideOp *__restrict__ ops, uint32_t n, unsigned long long *cl, uint32_t *sst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SideOp o = ops[i];
    if (o.bits & SIDE_POS) atomicMax(&cl[2 * (size_t)o.slot], o.claim);
    if (o.bits & SIDE_YAW) atomicMax(&cl[2 * (size_t)o.slot + 1], o.claim);
    if (o.bits & SIDE_SIF) atomicOr(&sst[SLOT_W * (size_t)o.slot + SST_FLAGS], o.bits & SIDE_SIF);
}

__global__ void k_side_write(const SideOp *__restrict__ ops, uint32_t n, const unsigned long long *cl, float4 *pos) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SideOp o = ops[i];
    float *p = reinterpret_cast<float *>(pos + SLOT_U4 * (size_t)o.slot);
    if ((o.bits & SIDE_POS) && cl[2 * (size_t)o.slot] == o.claim) {
        p[0] = o.pos.x;
        p[1] = o.pos.y;
        p[2] = o.pos.z;
    }
    if ((o.bits & SIDE_YAW) && cl[2 * (size_t)o.slot + 1] == o.claim) p[3] = o.pos.w;
}

// ------------------------------------------------------------- decode ------
struct DecodeArgs {
    const uint4 *pay;  // 2 uint4 per record: id, (x, y, z, yaw) bits
    uint32_t n;
    const uint4 *htab;
    uint32_t hmask;  // buckets - 1 (power of two)
    uint32_t *sst;
    uint32_t *o_slot, *o_sp;  // the device Moved batch (SLOT_NONE: no move)
    float *o_x, *o_z;
    uint32_t *o_ys;  // slot of an applied record (SLOT_NONE: skipped), for k_decode_yaw
    unsigned long long claim0;
    unsigned long long *cl;
    float4 *pos;
    uint32_t *oflag, *oflag_n;  // slots flagged outside every AOI space (own-client records)
    uint32_t *h_ndec;           // pinned host word: *oflag_n once the batch is decoded
    uint32_t oflag_cap;         // entries oflag holds (max_slots: one per slot, see k_decode)
    uint32_t *dups, *ndup;      // slots with a record whose claim store did not survive (1)
};

// The id table: 64-B buckets (one line), three entries each: keys in words 0..11,
// the three slots in words 12..14 (H_EMPTY never used, H_TOMB freed).  Linear
// probing over entries e = 3 b + way, so a probe reads one line per step and
// almost always stops in the first (half the bytes of the 32-B bucket layout).
// One bucket's three entries against id: true when the probe ends here (found, or an
// empty entry: not in the table), with the slot (or SLOT_NONE) in *out.
__device__ __forceinline__ bool probe_bucket(const uint4 (&k)[3], const uint4 &m, const uint4 &id, uint32_t *out) {
    const uint32_t v[3] = {m.x, m.y, m.z};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (v[q] == H_EMPTY) {
            *out = SLOT_NONE;
            return true;
        }
        if (v[q] != H_TOMB && eq4(k[q], id)) {
            *out = v[q];
            return true;
        }
    }
    return false;
}

__device__ __forceinline__ uint32_t lookup(const uint4 *__restrict__ htab, uint32_t bmask, uint4 id,
                                           uint32_t probe0 = 0) {
    uint32_t b = (id_hash(id.x, id.y, id.z, id.w) + probe0) & bmask;
    for (uint32_t probe = probe0; probe <= bmask; ++probe, b = (b + 1) & bmask) {
        uint4 k[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) k[q] = htab[4 * (size_t)b + (uint32_t)q];
        const uint4 m = htab[4 * (size_t)b + 3];
        const uint32_t v[3] = {m.x, m.y, m.z};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (v[q] == H_EMPTY) return SLOT_NONE;
            if (v[q] != H_TOMB && eq4(k[q], id)) return v[q];
        }
    }
    return SLOT_NONE;
}

// The record's effects once its slot is known (s: the looked-up slot or SLOT_NONE; st: its
// slot record when s != SLOT_NONE).
__device__ __forceinline__ void decode_rest(const DecodeArgs &A, uint32_t i, const uint4 &pv, uint32_t s,
                                            const uint4 &st) {
    uint32_t sp = SP_DEAD, old = 0;
    if (s != SLOT_NONE) {
        sp = st.y;  // SST_SPACE
        old = st.w;  // SST_FLAGS
        if (!st.z) s = SLOT_NONE;  // SST_SYNCING
    }
    const bool move = s != SLOT_NONE && sp != SP_DEAD;
    A.o_slot[i] = move ? s : SLOT_NONE;
    A.o_x[i] = __uint_as_float(pv.x);
    A.o_z[i] = __uint_as_float(pv.z);
    A.o_sp[i] = sp;
    A.o_ys[i] = s;
    if (s != SLOT_NONE) {
        // Plain stores, no atomics (a device-scope atomic is performed memory-side
        // on gfx950, ~17x slower than a store for 64 lanes on 64 lines): the
        // claims of this batch are larger than every claim already applied, so a
        // store replaces them; among records of one slot in this batch a random
        // store survives, and k_decode_fix folds the others in.
        const unsigned long long c = A.claim0 + i;
        if (move) reinterpret_cast<ulonglong2 *>(A.cl)[s] = make_ulonglong2(c, c);
        else A.cl[2 * (size_t)s + 1] = c;
        // (the flags word came with the slot's record; records of one slot all set the same bit)
        uint32_t *fl = A.sst + SLOT_W * (size_t)s + SST_FLAGS;
        if (!move && old == 0u) {
            // first flag of a slot outside the frame since the last collect: the flag is
            // claimed atomically, so a slot with several records in the batch is listed
            // once and the list never holds more than one entry per slot (rare path: only
            // entities outside every AOI space get here)
            if (atomicOr(fl, GWAOI_SIF_NEIGHBOR_CLIENTS) == 0u) {
                const uint32_t k = atomicAdd(A.oflag_n, 1u);
                if (k < A.oflag_cap) A.oflag[k] = s;
            }
        } else if (!(old & GWAOI_SIF_NEIGHBOR_CLIENTS)) {
            *fl = old | GWAOI_SIF_NEIGHBOR_CLIENTS;
        }
    }
}


// OnSyncPositionYawFromClient: unknown id -> skip (EntityManager.go:486-490);
// syncPositionYawFromClient: only if syncing (Entity.go:432).  setPositionYaw
// (Entity.go:1189-1205) then runs for every entity: e.Space is nilSpace, not
// nil, outside every space.  In an AOI space it is a Moved (op i of the
// batch) plus Position; elsewhere Space.move returns before Position
// (Space.go:253-257) and only yaw changes.  Both raise sifSyncNeighborClients.
// PER records per thread, strided by the block: every slot record is loaded before any is used.
#ifndef GWAOI_DEC_PER
#define GWAOI_DEC_PER 2  // records per k_decode thread (2: 102 vs 113 us at 1M records, profiles/archive/r04_variants_sync.log)
#endif
template <int PER>
__global__ __launch_bounds__(ST) void k_decode(DecodeArgs A) {
    const uint32_t i0 = blockIdx.x * (ST * PER) + threadIdx.x;
    if (i0 == 0) *A.ndup = 0u;  // read by k_decode_apply, the next launch on the stream
    uint4 id[PER], pv[PER];
    uint32_t s[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const uint32_t i = i0 + (uint32_t)u * ST;
        const size_t ic = i < A.n ? i : 0u;  // (clamped: the loads issue together)
        id[u] = A.pay[2 * ic];
        pv[u] = A.pay[2 * ic + 1];
    }
    // the first bucket of every record's probe in flight together (a probe almost always ends
    // there); the rare longer probe continues from the next bucket
    uint4 hk[PER][3], hm[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const size_t b = id_hash(id[u].x, id[u].y, id[u].z, id[u].w) & A.hmask;
#pragma unroll
        for (int q = 0; q < 3; ++q) hk[u][q] = A.htab[4 * b + (uint32_t)q];
        hm[u] = A.htab[4 * b + 3];
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        s[u] = SLOT_NONE;
        if (i0 + (uint32_t)u * ST < A.n && !probe_bucket(hk[u], hm[u], id[u], &s[u]))
            s[u] = lookup(A.htab, A.hmask, id[u], 1u);
    }
    uint4 st[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {  // every slot record in flight together (clamped slot: no branch)
        st[u] = reinterpret_cast<const uint4 *>(A.sst)[SLOT_U4 * (size_t)(s[u] != SLOT_NONE ? s[u] : 0u)];
        if (s[u] == SLOT_NONE) st[u] = make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const uint32_t i = i0 + (uint32_t)u * ST;
        if (i < A.n) decode_rest(A, i, pv[u], s[u], st[u]);
    }
}


// The claim fold and the apply in one pass.  A record whose claim store survived
// (cs == c) applies its position / yaw; one whose store was overwritten by another
// record of the same slot folds its claim in with atomicMax and lists the slot.
// Whatever the interleaving, every slot with two or more records in the batch is
// listed by one of them, and k_decode_dups then applies the record that holds the
// final (largest) claim.  A batch without repeated slots pays no atomic and
// lists nothing: the separate read-only fold pass (k_decode_fix) is gone.
__global__ __launch_bounds__(ST) void k_decode_apply(DecodeArgs A) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t s = A.o_ys[i];
    if (s == SLOT_NONE) return;
    const unsigned long long c = A.claim0 + i;
    const uint4 pv = A.pay[2 * (size_t)i + 1];
    float *p = reinterpret_cast<float *>(A.pos + SLOT_U4 * (size_t)s);
    const ulonglong2 cs = reinterpret_cast<const ulonglong2 *>(A.cl)[s];
    const bool moves = A.o_sp[i] != SP_DEAD;
    if (moves && cs.x == c && cs.y == c) {  // the common case: one 16-B store of position and yaw
        A.pos[SLOT_U4 * (size_t)s] = make_float4(__uint_as_float(pv.x), __uint_as_float(pv.y), __uint_as_float(pv.z),
                               __uint_as_float(pv.w));
        return;
    }
    bool lost = false;
    if (moves) {
        if (cs.x == c) {
            p[0] = __uint_as_float(pv.x);
            p[1] = __uint_as_float(pv.y);
            p[2] = __uint_as_float(pv.z);
        } else {
            atomicMax(&A.cl[2 * (size_t)s], c);
            lost = true;
        }
    }
    if (cs.y == c) {
        p[3] = __uint_as_float(pv.w);
    } else {
        atomicMax(&A.cl[2 * (size_t)s + 1], c);
        lost = true;
    }
    if (lost) A.dups[atomicAdd(A.ndup, 1u)] = s;
}

// Listed slots (rare; may repeat): apply the records holding the final claims.
__global__ __launch_bounds__(ST) void k_decode_dups(DecodeArgs A) {
    const uint32_t nd = *A.ndup;
    if (blockIdx.x == 0 && threadIdx.x == 0) *A.h_ndec = *A.oflag_n;  // (for the collect, no copy)
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nd; k += gridDim.x * blockDim.x) {
        const uint32_t s = A.dups[k];
        const ulonglong2 cs = reinterpret_cast<const ulonglong2 *>(A.cl)[s];
        float *p = reinterpret_cast<float *>(A.pos + SLOT_U4 * (size_t)s);
        const unsigned long long ix = cs.x - A.claim0, iy = cs.y - A.claim0;  // claims of older batches wrap
        if (ix < A.n && A.o_ys[ix] == s && A.o_sp[ix] != SP_DEAD) {
            const uint4 pv = A.pay[2 * (size_t)ix + 1];
            p[0] = __uint_as_float(pv.x);
            p[1] = __uint_as_float(pv.y);
            p[2] = __uint_as_float(pv.z);
        }
        if (iy < A.n && A.o_ys[iy] == s) p[3] = __uint_as_float(A.pay[2 * (size_t)iy + 1].w);
    }
}

// ------------------------------------------------------------ fan-out ------
// Receiver side: CollectEntitySyncInfos sends entity A's record to the client
// of every B in A.InterestedBy, i.e. every B with rel(A,B).  One lane per
// frame entity B with a client (gate g): its records are its own one (if B's
// sifSyncOwnClient is set) plus one per A in B's window with rel(A,B) and
// sifSyncNeighborClients set on A.  All of a lane's records go to one gate,
// so a lane reserves its whole run with one LDS atomic and writes it
// contiguously.  k_fan_prep first lays the senders out in frame order
// (flags, id, position/yaw) so that the window walk reads them next to the
// frame records, and clears the flags.
struct FanArgs {
    FrameView F;
    SlotTab info;  // slot -> frame index (rank) of the world
    const uint32_t *left;  // flagged slots outside the frame (own-client records only), may repeat
    uint32_t n_left;
    const uint4 *eid, *cid;
    uint32_t *sst;
    const float4 *pos;
    // frame-ordered (n + n_left entries), written by k_fan_prep
    uint32_t *snd;    // sender flags
    uint32_t *rg;     // receiver gate (NO_GATE: no client)
    uint4 *srec;      // 2 per entry: sender id, then x, y, z, yaw (one 32-B load per record)
    uint4 *frec;      // frame records (x, z, seq) with sifSyncNeighborClients in bit 63
    uint4 *fcid;      // receiver's ClientID (entries with a client; from the slot record's line)
    uint32_t *fcnt, *fsb;  // records of each entry, its run in the scratch
    uint32_t *scr;         // hits: sender entry of each record, receiver-contiguous runs
    unsigned long long *scr_cursor;
    unsigned long long scr_cap;  // < SCR_FULL
    uint32_t G, nb;
    uint32_t *blk_cnt;  // [G][nb] (pass 1 writes, the scan turns it into bases)
    uint4 *out;         // 3 uint4 per record (pass 2)
    unsigned long long out_recs;  // records out holds (pass 2 writes nothing past a larger total)
};

__global__ __launch_bounds__(ST) void k_fan_prep(FanArgs A) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nf = A.F.n;
    if (i == 0) {  // the hits pass's scratch cursor and the scan's extra count (first attempt)
        *A.scr_cursor = 0ull;
        A.blk_cnt[(size_t)A.G * A.nb] = 0u;
    }
    if (i >= nf + A.n_left) return;
    const bool in_frame = i < nf;
    const uint32_t s = in_frame ? ld_ss(A.F.ss, i).slot : A.left[i - nf];
    // the slot's whole 64-B record and the frame record, all loaded before any is used (a load
    // under a per-lane branch is waited for before the next one issues)
    const uint4 *rec = reinterpret_cast<const uint4 *>(A.sst) + SLOT_U4 * (size_t)s;
    const uint4 st = rec[0];  // gate, space, syncing, flags
    const uint4 pw = rec[1];  // Position, yaw
    const uint4 id = rec[2];  // EntityID
    const uint4 ci = rec[3];  // ClientID
    const uint4 q = reinterpret_cast<const uint4 *>(A.F.rec)[in_frame ? i : 0u];
    uint32_t fl;
    if (in_frame) {
        fl = st.w;
        if (fl) A.sst[SLOT_W * (size_t)s + SST_FLAGS] = 0u;
    } else {
        // a listed slot back in the frame is its frame entry's; a slot listed twice is sent once
        const uint32_t r = A.info.rank[s];
        fl = (r < nf && ld_ss(A.F.ss, r).slot == s) ? 0u : atomicExch(&A.sst[SLOT_W * (size_t)s + SST_FLAGS], 0u);
    }
    A.snd[i] = fl;
    A.rg[i] = st.x;
    A.fcid[i] = ci;  // (the receiver's, read in frame order by the write pass)
    if (in_frame) {  // the walk's candidate record: x, z, seq with the sender flag in bit 63
        uint4 f = q;
        if (fl & GWAOI_SIF_NEIGHBOR_CLIENTS) f.w |= 0x80000000u;
        A.frec[i] = f;
    }
    if (fl) {
        // the frame holds the AOI position; outside the frame, the last Position written
        const uint32_t x = in_frame ? q.x : pw.x, z = in_frame ? q.y : pw.z;
        A.srec[2 * (size_t)i] = id;
        A.srec[2 * (size_t)i + 1] = make_uint4(x, pw.y, z, pw.w);
    }
}

__device__ __forceinline__ uint32_t s_lane() { return __lane_id(); }

// Exclusive scan of n (<= ST * k) LDS words in place by one workgroup.
__device__ void lds_excl_scan(uint32_t *a, uint32_t n, uint32_t *ws) {
    const uint32_t k = (n + ST - 1) / ST, b = threadIdx.x * k;
    uint32_t sum = 0;
    for (uint32_t q = 0; q < k && b + q < n; ++q) sum += a[b + q];
    uint32_t x = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if ((int)s_lane() >= o) x += y;
    }
    const uint32_t w = threadIdx.x / 64;
    if (s_lane() == 63) ws[w] = x;
    __syncthreads();
    uint32_t pre = x - sum;
    for (uint32_t q = 0; q < w; ++q) pre += ws[q];
    for (uint32_t q = 0; q < k && b + q < n; ++q) {
        const uint32_t v = a[b + q];
        a[b + q] = pre;
        pre += v;
    }
    __syncthreads();
}

// Block-wide exclusive scan of one value per thread (ST threads).
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t *ws, uint32_t &total) {
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if ((int)s_lane() >= o) x += y;
    }
    const uint32_t w = threadIdx.x / 64;
    if (s_lane() == 63) ws[w] = x;
    __syncthreads();
    uint32_t pre = x - v;
    total = 0;
    for (uint32_t q = 0; q < ST / 64; ++q) {
        if (q < w) pre += ws[q];
        total += ws[q];
    }
    __syncthreads();
    return pre;
}

// The go-aoi window of receiver entry i (cells), widened by the float32
// rounding margin of the window bounds.
struct FanWin {
    Rec16 R;
    float D;
    uint32_t row0, gx;  // cell index of (cx0, cz0), grid row length
    int cx0, cx1, cz0, cz1;
};
__device__ __forceinline__ FanWin fan_window(const FrameView &F, uint32_t i) {
    FanWin W;
    W.R = ld_rec(F.rec, i);
    const SpaceGrid gr = F.grid[ld_ss(F.ss, i).sp];
    W.D = gr.D;
    const float mx = (fabsf(W.R.x) + 3.0f * W.D) * 0x1p-20f, mz = (fabsf(W.R.z) + 3.0f * W.D) * 0x1p-20f;
    W.cx0 = cell_of(W.R.x - W.D - mx, gr.ox, gr.inv, gr.gx);
    W.cx1 = cell_of(W.R.x + W.D + mx, gr.ox, gr.inv, gr.gx);
    W.cz0 = cell_of(W.R.z - W.D - mz, gr.oz, gr.inv, gr.gz);
    W.cz1 = cell_of(W.R.z + W.D + mz, gr.oz, gr.inv, gr.gz);
    W.gx = gr.gx;
    W.row0 = gr.base + (uint32_t)W.cz0 * gr.gx + (uint32_t)W.cx0;
    return W;
}

// Fan-out pass 1 (hits).  Entry i (frame order, then the listed slots outside
// the frame) with a client is a receiver: it lists the senders of its records
// in the scratch, itself first if sifSyncOwnClient, then every A in its go-aoi
// window with sifSyncNeighborClients and rel(A,B), rows in order and frame
// order inside a row.  Its scratch run is sized by the window's candidate
// count (one lane per entry, cell_start loads only) and placed by one atomic
// per block, so the window is walked once; a block past the scratch capacity
// writes no hits (the host regrows the scratch and reruns this pass; it has no
// other side effect).  The walk takes a wave per receiver (FAN_NR of a wave's
// receivers at a time): the window rows are laid end to end (lane j loads row
// j's bounds; a DPP scan gives each row's first position) and the wave deals
// out 64 consecutive positions per step.  A lane's candidate is found from the
// rows starting in the step (an LDS mark per position, a ballot) and the row's
// offset (LDS), so one load instruction reads 64 consecutive candidates instead
// of one candidate from each of 64 windows (the round-5 lane-per-receiver walk:
// 353 against 249 us, profiles/r06_ab_fan_hits.txt), and the hits are
// compacted by a ballot into consecutive 4-B stores.
#ifndef GWAOI_FAN_WU
#define GWAOI_FAN_WU 2  // steps of 64 positions per receiver with their loads in flight together
#endif
constexpr int FAN_WU = GWAOI_FAN_WU;
#ifndef GWAOI_FAN_NR
#define GWAOI_FAN_NR 2  // receivers of a wave dealt together (A/B, profiles/r06_ab_fan_hits.txt: k_fan_hits
                        // 252 us at NR 2 / WU 2, 259 at 3 / 2, 279 at 4 / 2, 283 at 2 / 4, 267 at 1 / 4)
#endif
constexpr int FAN_NR = GWAOI_FAN_NR;
#ifndef GWAOI_FAN_UBU
#define GWAOI_FAN_UBU 4  // window rows whose bounds the run sizing loads together
#endif
constexpr int FAN_UBU = GWAOI_FAN_UBU;

__device__ __forceinline__ uint32_t rdl(uint32_t v, uint32_t k) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)k);
}

__global__ __launch_bounds__(ST) void k_fan_hits_wave(FanArgs A) {
    extern __shared__ uint32_t gcnt[];  // [G] records per gate of the block
    __shared__ uint32_t s_ws[ST / 64];
    __shared__ uint32_t s_base;
    __shared__ uint32_t s_adj[ST / 64][FAN_NR][64];            // candidate index - position, per non-empty row
    __shared__ uint32_t s_mark[ST / 64][FAN_NR][FAN_WU * 64];  // a non-empty row starts at this position
    const uint32_t blk = xcd_block(blockIdx.x, gridDim.x);
    const uint32_t nf = A.F.n, ne = nf + A.n_left;
    const uint32_t w = threadIdx.x / 64, ln = s_lane();
    for (uint32_t q = threadIdx.x; q < A.G; q += blockDim.x) gcnt[q] = 0u;
    const uint32_t i = blk * ST + threadIdx.x;
    const uint32_t g = i < ne ? A.rg[i] : NO_GATE;
    const bool on = g != NO_GATE;
    const bool own = on && (A.snd[i] & GWAOI_SIF_OWN_CLIENT);
    const bool walk = on && i < nf;
    const uint32_t *cs = A.F.cell_start;
    FanWin W{};
    uint32_t ub = own ? 1u : 0u;
    if (walk) {
        W = fan_window(A.F, i);
        const uint32_t span = (uint32_t)(W.cx1 - W.cx0) + 1u;
        for (int cz = W.cz0; cz <= W.cz1; cz += FAN_UBU) {  // FAN_UBU rows' bounds in flight together
            uint32_t lo[FAN_UBU], hi[FAN_UBU];
#pragma unroll
            for (int u = 0; u < FAN_UBU; ++u) {
                const uint32_t rb = W.row0 + (uint32_t)(min(cz + u, W.cz1) - W.cz0) * W.gx;
                lo[u] = cs[rb];
                hi[u] = cs[rb + span];
            }
#pragma unroll
            for (int u = 0; u < FAN_UBU; ++u)
                if (cz + u <= W.cz1) ub += hi[u] - lo[u];
        }
    }
    ub = (ub + 3u) & ~3u;  // (runs start 16-B aligned)
    uint32_t tot;
    const uint32_t off = block_excl(ub, s_ws, tot);
    if (threadIdx.x == 0) {
        const unsigned long long b = tot ? atomicAdd(A.scr_cursor, (unsigned long long)tot) : 0ull;
        s_base = b + tot <= A.scr_cap ? (uint32_t)b : SCR_FULL;
    }
    __syncthreads();
    const bool fits = s_base != SCR_FULL;
    const uint32_t sb = s_base + off;
    if (own && fits) A.scr[sb] = i;
    uint32_t c = own ? 1u : 0u;
    const unsigned long long lt = (1ull << ln) - 1ull;
    const unsigned long long le = ln == 63 ? ~0ull : (2ull << ln) - 1ull;
    unsigned long long todo = __ballot(walk);
#ifdef GWAOI_EXP_FAN_NOWALK  // timing only: the run sizing and placement without the walks (no neighbour records)
    todo = 0;
#endif
    while (todo) {
        // FAN_NR receivers at a time, their steps interleaved (a receiver's chain of row-bound
        // loads, then candidate loads, is latency-bound alone); a missing one has no rows
        uint32_t k[FAN_NR], ri[FAN_NR], row0[FAN_NR], gx[FAN_NR], span[FAN_NR], nrows[FAN_NR], rsb[FAN_NR],
            rc[FAN_NR];
        float rx[FAN_NR], rz[FAN_NR], D[FAN_NR];
        unsigned long long rs[FAN_NR];
        uint32_t maxrows = 0;
#pragma unroll
        for (int r = 0; r < FAN_NR; ++r) {
            k[r] = todo ? (uint32_t)__builtin_ctzll(todo) : 64u;
            todo &= todo - 1ull;
            const uint32_t kk = min(k[r], 63u);
            ri[r] = blk * ST + w * 64u + kk;
            rx[r] = __uint_as_float(rdl(__float_as_uint(W.R.x), kk));
            rz[r] = __uint_as_float(rdl(__float_as_uint(W.R.z), kk));
            D[r] = __uint_as_float(rdl(__float_as_uint(W.D), kk));
            rs[r] = ((unsigned long long)rdl((uint32_t)(W.R.s >> 32), kk) << 32) | rdl((uint32_t)W.R.s, kk);
            row0[r] = rdl(W.row0, kk);
            gx[r] = rdl(W.gx, kk);
            span[r] = rdl((uint32_t)(W.cx1 - W.cx0), kk) + 1u;
            nrows[r] = k[r] < 64u ? rdl((uint32_t)(W.cz1 - W.cz0), kk) + 1u : 0u;
            rsb[r] = rdl(sb, kk);
            rc[r] = rdl(c, kk);
            maxrows = max(maxrows, nrows[r]);
        }
        for (uint32_t j0 = 0; j0 < maxrows; j0 += 64u) {
            // lane t: row j0 + t of each window, its candidates [jb, jb + len)
            const uint32_t t = j0 + ln;
            uint32_t jb[FAN_NR], je[FAN_NR], len[FAN_NR], ex[FAN_NR], T[FAN_NR];
#pragma unroll
            for (int r = 0; r < FAN_NR; ++r) {
                const uint32_t rb = row0[r] + min(t, max(nrows[r], 1u) - 1u) * gx[r];
                jb[r] = cs[rb];
                je[r] = cs[rb + span[r]];
            }
            uint32_t Tm = 0;
#pragma unroll
            for (int r = 0; r < FAN_NR; ++r) {
                len[r] = t < nrows[r] ? je[r] - jb[r] : 0u;
                const uint32_t incl = wave_scan_add(len[r]);
                ex[r] = incl - len[r];
                T[r] = rdl(incl, 63);
                Tm = max(Tm, T[r]);
                const unsigned long long nem = __ballot(len[r] != 0u);
                if (len[r]) s_adj[w][r][__popcll(nem & lt)] = jb[r] - ex[r];
            }
            for (uint32_t p0 = 0; p0 < Tm; p0 += FAN_WU * 64u) {
#pragma unroll
                for (int r = 0; r < FAN_NR; ++r)
#pragma unroll
                    for (int u = 0; u < FAN_WU; ++u) s_mark[w][r][u * 64 + ln] = 0u;
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                uint32_t nr[FAN_NR];  // non-empty rows started before this step
#pragma unroll
                for (int r = 0; r < FAN_NR; ++r) {
                    if (len[r] && ex[r] >= p0 && ex[r] - p0 < FAN_WU * 64u) s_mark[w][r][ex[r] - p0] = 1u;
                    nr[r] = (uint32_t)__popcll(__ballot(len[r] != 0u && ex[r] < p0));
                }
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                uint32_t b[FAN_NR][FAN_WU];
                uint4 q[FAN_NR][FAN_WU];
#pragma unroll
                for (int r = 0; r < FAN_NR; ++r)
#pragma unroll
                    for (int u = 0; u < FAN_WU; ++u) {
                        const unsigned long long m = __ballot(s_mark[w][r][u * 64 + ln] != 0u);
                        const uint32_t p = p0 + (uint32_t)u * 64u + ln;
                        const uint32_t row = nr[r] + (uint32_t)__popcll(m & le);  // rows started at or before p
                        nr[r] += (uint32_t)__popcll(m);
                        b[r][u] = p < T[r] ? p + s_adj[w][r][row - 1u] : ri[r];  // (row >= 1 whenever p < T)
                        q[r][u] = A.frec[b[r][u]];
                    }
#pragma unroll
                for (int r = 0; r < FAN_NR; ++r)
#pragma unroll
                    for (int u = 0; u < FAN_WU; ++u) {
                        const uint32_t p = p0 + (uint32_t)u * 64u + ln;
                        const uint4 &Q = q[r][u];
                        const unsigned long long bs = ((unsigned long long)(Q.w & 0x7FFFFFFFu) << 32) | Q.z;
                        const bool hit = p < T[r] && b[r][u] != ri[r] && (Q.w >> 31) &&
                                         rel(rx[r], rz[r], rs[r], __uint_as_float(Q.x), __uint_as_float(Q.y), bs, D[r]);
                        const unsigned long long hm = __ballot(hit);
                        if (hit && fits) A.scr[rsb[r] + rc[r] + (uint32_t)__popcll(hm & lt)] = b[r][u];
                        rc[r] += (uint32_t)__popcll(hm);
                    }
            }
            __builtin_amdgcn_wave_barrier();  // s_adj is rewritten by the next row group
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        }
#pragma unroll
        for (int r = 0; r < FAN_NR; ++r)
            if (ln == k[r]) c = rc[r];
    }
    if (i < ne) {
        A.fcnt[i] = c;
        A.fsb[i] = sb;
    }
    if (c) atomicAdd(&gcnt[g], c);
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < A.G; q += blockDim.x) A.blk_cnt[(size_t)q * A.nb + blk] = gcnt[q];
}

// Fan-out pass 2 (write): block blk expands the hits of its receivers into
// 48-B records (receiver's ClientID, sender's EntityID, x, y, z, yaw).  The
// receivers are regrouped by gate (stable), so the block's records of gate g
// form one run starting at the scanned base of (g, blk).  Thread t writes
// records t, t + ST, ... of the block: consecutive threads write consecutive
// records of a run (coalesced stores), each finding its receiver by a binary
// search of the inclusive record prefix in LDS.  (GoWorld's own per-gate
// order is Go map order, EntityManager.go's entity loop: the order of
// records inside a gate is not part of the contract.)
#ifndef GWAOI_FW_G
#define GWAOI_FW_G 12  // A/B (profiles/r06_ab_fan_write.txt): collect 1.355 (4), 1.285 (6), 1.242 (8), 1.203 (12), 1.210 (16) ms once the hit loads stopped serialising
#endif
constexpr int FW_G = GWAOI_FW_G;  // record groups of 64 per wave with their loads in flight together

__global__ __launch_bounds__(ST) void k_fan_write(FanArgs A) {
    extern __shared__ uint32_t lds[];  // bin[G + 1] | gbase[G] | seg[G]
    __shared__ uint32_t s_pre[ST], s_sb[ST], s_gate[ST];
    __shared__ uint4 s_cli[ST];
    __shared__ uint4 s_rec[ST / 64][3 * 64];  // a wave's 64 records, staged for contiguous stores
    __shared__ uint32_t s_pos[ST / 64][64];
    __shared__ uint32_t s_ws[ST / 64];
    // launched behind the hits pass without a host round trip: nothing to do when the hits
    // overflowed the scratch or the total (the scan's last entry) outgrew the output; the host
    // sees both after its one sync and reruns
    if (*A.scr_cursor > A.scr_cap || A.blk_cnt[(size_t)A.G * A.nb] > A.out_recs) return;
    uint32_t *bin = lds, *gbase = lds + A.G + 1, *seg = gbase + A.G;
    const uint32_t blk = xcd_block(blockIdx.x, gridDim.x);
    const uint32_t ne = A.F.n + A.n_left;
    const uint32_t w = threadIdx.x / 64, ln = s_lane();
    for (uint32_t q = threadIdx.x; q <= A.G; q += blockDim.x) bin[q] = 0u;
    for (uint32_t q = threadIdx.x; q < A.G; q += blockDim.x) gbase[q] = A.blk_cnt[(size_t)q * A.nb + blk];
    __syncthreads();
    const uint32_t i = blk * ST + threadIdx.x;
    // the receiver's gate, record count, run and ClientID in one round trip (clamped index, no
    // load under a branch)
    const uint32_t ic = i < ne ? i : 0u;
    const uint32_t g0 = A.rg[ic], cnt0 = A.fcnt[ic], sb0 = A.fsb[ic];
    const uint4 cli = A.fcid[ic];
    const uint32_t g = i < ne ? g0 : NO_GATE;
    const uint32_t key = g == NO_GATE ? A.G : g;
    const uint32_t r0 = atomicAdd(&bin[key], 1u);
    __syncthreads();
    lds_excl_scan(bin, A.G + 1, s_ws);
    const uint32_t p = bin[key] + r0;  // (the order inside a gate's run is not part of the contract)
    const uint32_t c = g != NO_GATE ? cnt0 : 0u;
    s_pre[p] = c;
    s_sb[p] = c ? sb0 : 0u;
    s_gate[p] = key;
    if (c) s_cli[p] = cli;
    __syncthreads();
    uint32_t R;
    const uint32_t mine = s_pre[threadIdx.x];
    const uint32_t ex = block_excl(mine, s_ws, R);
    s_pre[threadIdx.x] = ex + mine;  // inclusive
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < A.G; q += blockDim.x) seg[q] = bin[q] ? s_pre[bin[q] - 1] : 0u;
    __syncthreads();
    const uint4 *srec = A.srec;
    // record r of receiver q -> (its scratch entry, output position)
    auto place = [&](uint32_t r, uint32_t q, uint32_t &sidx, uint32_t &pos) {
        const uint32_t gq = s_gate[q];
        sidx = s_sb[q] + r - (q ? s_pre[q - 1] : 0u);
        pos = gbase[gq] + (r - seg[gq]);
    };
    auto search = [&](uint32_t r) {  // first receiver q with s_pre[q] > r
        uint32_t lo = 0, hi = ST - 1;
        while (lo < hi) {
            const uint32_t m = (lo + hi) >> 1;
            if (s_pre[m] > r) hi = m;
            else lo = m + 1;
        }
        return lo;
    };
    // stage a wave's 64 records in LDS, then store them as 3 x 64 consecutive 16-B words
    auto emit = [&](uint32_t nrec, bool ok, uint32_t q, uint32_t pos, const uint4 &id, const uint4 &pv) {
        if (ok) {
            s_pos[w][ln] = pos;
            s_rec[w][3 * ln] = s_cli[q];
            s_rec[w][3 * ln + 1] = id;
            s_rec[w][3 * ln + 2] = pv;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) {
            const uint32_t e = ln + 64u * j, rr = e / 3u;
            if (rr < nrec)
                st_stream(A.out + 3 * (size_t)s_pos[w][rr] + (e - 3u * rr), s_rec[w][e]);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    };
    // wave w: one contiguous chunk [c0, c1) of the block's records, FW_G consecutive groups of 64
    // per step with all groups' loads in flight.  A lane's records are then exactly 64 apart
    // (under one receiver on average), so its receiver is found by a forward scan from the last
    // one instead of a binary search over the block per record.
    const uint32_t per = (R + ST - 1u) / ST * 64u;  // ST / 64 waves
    const uint32_t c0 = min(R, w * per), c1 = min(R, c0 + per);
    uint32_t qc = c0 + ln < c1 ? search(c0 + ln) : 0u;
    for (uint32_t rw = c0; rw < c1; rw += FW_G * 64) {
        uint32_t q[FW_G], pos[FW_G], h[FW_G];
        bool ok[FW_G];
#pragma unroll
        for (int k = 0; k < FW_G; ++k) {
            const uint32_t r = rw + (uint32_t)k * 64u + ln;
            ok[k] = r < c1;
            uint32_t sidx = 0;
            q[k] = pos[k] = 0;
            if (ok[k]) {
                while (s_pre[qc] <= r) ++qc;  // ends: s_pre[ST - 1] = R > r
                q[k] = qc;
                place(r, qc, sidx, pos[k]);
            }
            h[k] = A.scr[sidx];  // (sidx 0 when !ok: a load under a per-lane branch is waited for
        }                        // before the next one issues, which serialised the groups)
        uint4 id[FW_G], pv[FW_G];
#pragma unroll
        for (int k = 0; k < FW_G; ++k) {
            id[k] = pv[k] = make_uint4(0, 0, 0, 0);
            if (ok[k]) {
                id[k] = srec[2 * (size_t)h[k]];
                pv[k] = srec[2 * (size_t)h[k] + 1];
            }
        }
#pragma unroll
        for (int k = 0; k < FW_G; ++k) {
            const uint32_t rk = rw + (uint32_t)k * 64u;
            if (rk < c1) emit(min(64u, c1 - rk), ok[k], q[k], pos[k], id[k], pv[k]);
        }
    }
}

// ---------------------------------------------------------- broadcast ------
// Source side: GoWorld's AllClients delivery (Entity.CallAllClients, ForAllClients and the
// sendMapAttr* / sendListAttr* ...ToClients functions, Entity.go:743-917) for a sparse batch of
// messages.  Message m = (source slot, flags) yields one 32-B record {ClientID, m, source slot,
// receiver slot, 0} for the source's own client (GWAOI_CAST_OWN) and one for the client of
// every B with rel(source, B) (GWAOI_CAST_NEIGHBORS: B in the source's InterestedBy), grouped
// by the receiver's gate.  One wave per message; a block takes a contiguous chunk of messages,
// its waves every fourth one.  The source's window is walked twice and no hit list is kept:
// k_cast_count counts the block's records per gate in LDS, the scan gives every (gate, block)
// its base, k_cast_write repeats the walk (one body, cast_pass) and a hit takes the next
// position of its gate's run from an LDS cursor.  The walk (window_walk, shared with the client
// switch) is k_fan_hits_wave's: lane j loads
// row j's bounds, the rows are laid end to end and the wave reads 64 consecutive candidates
// per step; only hits go on to the candidate's slot and the first 16 B of its slot record
// (the gate), the other lanes re-read the source's (clamped index: no load under a per-lane
// branch).  Nothing is written but the counts and the output.
constexpr int CAST_WU = 2;  // steps of 64 candidates with their loads in flight together
constexpr uint32_t CAST_MAX_BLOCKS = 2048;  // the [G][nb] count table: 8 MB at 1,024 gates
constexpr unsigned long long CAST_E_SLOT = 1ull << 62;   // device form: a message's slot >= max_slots
constexpr unsigned long long CAST_E_FLAGS = 1ull << 63;  // device form: a flag bit outside OWN | NEIGHBORS
constexpr unsigned long long CAST_TOTAL = CAST_E_SLOT - 1ull;

struct CastArgs {
    FrameView F;
    SlotTab info;
    const uint4 *slots;       // SLOT_U4 per slot: sst, pos, eid, cid
    const uint32_t *m_slot;   // the messages' source slots
    const uint32_t *m_flags;  // their flags (nullptr: OWN | NEIGHBORS for every message)
    uint32_t n, max_slots;
    uint32_t G, nb, per;  // gates, blocks, messages per block
    uint32_t *blk_cnt;    // [G][nb] (the count pass writes, the scan turns it into bases)
    unsigned long long *sc;  // records of all blocks (64-bit: the scan's total wraps) | CAST_E_*
    uint4 *out;              // 2 uint4 per record (write pass)
    unsigned long long out_recs;  // records out holds (the write pass writes nothing past a larger total)
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// One wave walks the go-aoi window of the source at frame index r0 (record R, slot-space S0):
// exactly fan_window's cells (the same float32 margin, in the source's own space grid), lane j
// loads row j's bounds, the rows are laid end to end and the wave reads 64 consecutive
// candidates per step, CAST_WU steps with their loads in flight together.  After each group of
// steps step(b, q, hit) runs with every lane active: lane ln's candidate of step u is frame
// index b[u] with frame record q[u]; hit[u] is rel(source, candidate), never the source itself;
// a lane past the window's end has b[u] == r0 and no hit.  Shared by the broadcast and the
// client switch (wave w of the block, lane ln).
template <class Step>
__device__ __forceinline__ void window_walk(const FrameView &F, uint32_t r0, const Rec16 &R, const SlotSp &S0,
                                            uint32_t w, uint32_t ln, Step &&step) {
    __shared__ uint32_t s_adj[ST / 64][64];             // candidate index - position, per non-empty row
    __shared__ uint32_t s_mark[ST / 64][CAST_WU * 64];  // a non-empty row starts at this position
    const uint32_t *cs = F.cell_start;
    const uint4 *frec = reinterpret_cast<const uint4 *>(F.rec);
    const unsigned long long lt = (1ull << ln) - 1ull;
    const unsigned long long le = ln == 63 ? ~0ull : (2ull << ln) - 1ull;
    const SpaceGrid gr = F.grid[rfl(S0.sp)];
    const float D = gr.D;
    const float mx = (fabsf(R.x) + 3.0f * D) * 0x1p-20f, mz = (fabsf(R.z) + 3.0f * D) * 0x1p-20f;
    const int cx0 = cell_of(R.x - D - mx, gr.ox, gr.inv, gr.gx), cx1 = cell_of(R.x + D + mx, gr.ox, gr.inv, gr.gx);
    const int cz0 = cell_of(R.z - D - mz, gr.oz, gr.inv, gr.gz), cz1 = cell_of(R.z + D + mz, gr.oz, gr.inv, gr.gz);
    const uint32_t span = rfl((uint32_t)(cx1 - cx0) + 1u), nrows = rfl((uint32_t)(cz1 - cz0) + 1u);
    const uint32_t row0 = rfl(gr.base + (uint32_t)cz0 * gr.gx + (uint32_t)cx0), gx = rfl(gr.gx);
    for (uint32_t j0 = 0; j0 < nrows; j0 += 64u) {
        // lane t: row j0 + t of the window, its candidates [jb, je)
        const uint32_t t = j0 + ln;
        const uint32_t rb = row0 + min(t, nrows - 1u) * gx;
        const uint32_t jb = cs[rb], je = cs[rb + span];
        const uint32_t len = t < nrows ? je - jb : 0u;
        const uint32_t incl = wave_scan_add(len);
        const uint32_t ex = incl - len, T = rdl(incl, 63);
        const unsigned long long nem = __ballot(len != 0u);
        if (len) s_adj[w][__popcll(nem & lt)] = jb - ex;
        for (uint32_t p0 = 0; p0 < T; p0 += CAST_WU * 64u) {
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) s_mark[w][u * 64 + ln] = 0u;
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            if (len && ex >= p0 && ex - p0 < CAST_WU * 64u) s_mark[w][ex - p0] = 1u;
            uint32_t nr = (uint32_t)__popcll(__ballot(len != 0u && ex < p0));  // non-empty rows started before this step
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            uint32_t b[CAST_WU];
            uint4 q[CAST_WU];
            bool hit[CAST_WU];
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) {
                const unsigned long long mk = __ballot(s_mark[w][u * 64 + ln] != 0u);
                const uint32_t p = p0 + (uint32_t)u * 64u + ln;
                const uint32_t row = nr + (uint32_t)__popcll(mk & le);  // rows started at or before p
                nr += (uint32_t)__popcll(mk);
                b[u] = p < T ? p + s_adj[w][row - 1u] : r0;  // (row >= 1 whenever p < T)
                q[u] = frec[b[u]];
            }
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) {
                const uint32_t p = p0 + (uint32_t)u * 64u + ln;
                const unsigned long long bs = ((unsigned long long)q[u].w << 32) | q[u].z;
                hit[u] = p < T && b[u] != r0 &&  // (the source is never its own neighbour)
                         rel(R.x, R.z, R.s, __uint_as_float(q[u].x), __uint_as_float(q[u].y), bs, D);
            }
            step(b, q, hit);
        }
        __builtin_amdgcn_wave_barrier();  // s_adj is rewritten by the next row group
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
}

template <bool WRITE>
__device__ __forceinline__ void cast_pass(const CastArgs &A) {
    extern __shared__ uint32_t gcur[];  // [G] count: the block's records per gate; write: next position of its run
    __shared__ unsigned long long s_tot;
    // queued behind the count pass without a host round trip: nothing to do when the total outgrew
    // the output (the host sees it after its one sync, regrows and relaunches)
    if (WRITE && (*A.sc & CAST_TOTAL) > A.out_recs) return;
    const uint32_t blk = blockIdx.x, w = threadIdx.x / 64, ln = s_lane();
    for (uint32_t q = threadIdx.x; q < A.G; q += blockDim.x) gcur[q] = WRITE ? A.blk_cnt[(size_t)q * A.nb + blk] : 0u;
    if (!WRITE && threadIdx.x == 0) s_tot = 0ull;
    __syncthreads();
    unsigned long long wtot = 0ull, werr = 0ull;  // (wave-uniform)
    const uint32_t m1 = min(A.n, (blk + 1u) * A.per);
    for (uint32_t m = blk * A.per + w; m < m1; m += ST / 64) {
        const uint32_t slot = rfl(A.m_slot[m]);
        const uint32_t fl = A.m_flags ? rfl(A.m_flags[m]) : (GWAOI_CAST_OWN | GWAOI_CAST_NEIGHBORS);
        if (slot >= A.max_slots) {  // (device form only: the host form is checked on the host)
            werr |= CAST_E_SLOT;
            continue;
        }
        if (fl & ~(GWAOI_CAST_OWN | GWAOI_CAST_NEIGHBORS)) {
            werr |= CAST_E_FLAGS;
            continue;
        }
        if (!fl) continue;
        // the source: its frame index, gate and (write pass) ClientID in one round trip
        const uint32_t r0 = rfl(A.info.rank[slot]);
        const uint4 st0 = A.slots[SLOT_U4 * (size_t)slot];
        uint4 ci0 = make_uint4(0, 0, 0, 0);
        if (WRITE) ci0 = A.slots[SLOT_U4 * (size_t)slot + 3];
        // one record: its gate's count, or the next position of its gate's run and the two stores
        auto emit = [&](bool v, uint32_t g, uint32_t dst, const uint4 &cid) {
            v = v && g < A.G;  // (NO_GATE: no client)
            if (v) {
                const uint32_t p = atomicAdd(&gcur[g], 1u);
                if (WRITE && p < A.out_recs) {
                    A.out[2 * (size_t)p] = cid;
                    A.out[2 * (size_t)p + 1] = make_uint4(m, slot, dst, 0u);
                }
            }
            if (!WRITE) wtot += (unsigned long long)__popcll(__ballot(v));
        };
        // the own client's record whether or not the source is in an AOI space (e.client is
        // independent of the space; GameClient's methods are no-ops on a nil client)
        emit(ln == 0 && (fl & GWAOI_CAST_OWN), st0.x, slot, ci0);
        if (!(fl & GWAOI_CAST_NEIGHBORS) || r0 >= A.F.n) continue;  // (rank: 0xFFFFFFFF if never live)
        const SlotSp S0 = ld_ss(A.F.ss, r0);
        const Rec16 R = ld_rec(A.F.rec, r0);
        if (rfl(S0.slot) != slot) continue;  // left the frame: nilSpace or a space without AOI, no neighbours
        // the source's go-aoi window: only hits go on to the receiver's slot, then its gate (and
        // ClientID); every lane's load is issued (a lane without a hit re-reads the source's)
        window_walk(A.F, r0, R, S0, w, ln, [&](const uint32_t(&b)[CAST_WU], const uint4(&)[CAST_WU], const bool(&hit)[CAST_WU]) {
            uint32_t ds[CAST_WU];
            uint4 st[CAST_WU], ci[CAST_WU];
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) ds[u] = ld_ss(A.F.ss, hit[u] ? b[u] : r0).slot;
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) {
                st[u] = A.slots[SLOT_U4 * (size_t)ds[u]];
                ci[u] = make_uint4(0, 0, 0, 0);
                if (WRITE) ci[u] = A.slots[SLOT_U4 * (size_t)ds[u] + 3];
            }
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) emit(hit[u], st[u].x, ds[u], ci[u]);
        });
    }
    if (WRITE) return;
    if (ln == 0 && wtot) atomicAdd(&s_tot, wtot);
    if (ln == 0 && werr) atomicOr(A.sc, werr);  // (one lane per wave that saw a bad message)
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < A.G; q += blockDim.x) A.blk_cnt[(size_t)q * A.nb + blk] = gcur[q];
    if (threadIdx.x == 0) {
        if (s_tot) atomicAdd(A.sc, s_tot);  // one per block
        if (blk == 0) A.blk_cnt[(size_t)A.G * A.nb] = 0u;  // the scan's last entry becomes the (32-bit) total
    }
}

__global__ __launch_bounds__(ST) void k_cast_count(CastArgs A) { cast_pass<false>(A); }
__global__ __launch_bounds__(ST) void k_cast_write(CastArgs A) { cast_pass<true>(A); }

// ------------------------------------------------------ client switch ------
// Entity.SetClient for a batch (Entity.go:678-724; GiveClientTo, :752-765, is a detach of one
// entity and an attach of another).  Message m = (slot, new gate index or NO_GATE, new ClientID);
// the old client is the slot record's.  Unless the two are equal, every B with rel(source, B)
// (B in the source's InterestedBy, with or without a client) gives a 32-B destroy record {old
// ClientID, B's EntityID} under the old gate if there was a client, and a 48-B create record
// {new ClientID, B's EntityID, B's x, y, z, yaw: k_route's} under the new gate if there is one.
// The broadcast's shape: one wave per message, a block a contiguous chunk, the window walked by
// both passes (window_walk).  A message's two gates are wave-uniform, so the count pass loads
// nothing per hit: it adds the popcount of each step's hits in a register and the sum once per
// message to the block's LDS tables [2][G] (creates, then destroys, as k_route).  One scan
// over both parts; the write pass reads the split (all creates) from the scanned table.  It
// takes positions with one LDS atomic per table and wave step (lane 0 adds the popcount, a hit
// adds its rank among the hits) and only then loads B's slot, EntityID and position record.
// The clients themselves are changed after the write pass (k_switch_apply, from the same upload).
struct SwitchArgs {
    FrameView F;
    SlotTab info;
    const uint4 *slots;      // SLOT_U4 per slot: sst, pos, eid, cid
    const uint4 *m_cid;      // the messages' new ClientIDs
    const uint32_t *m_slot;  // their slots
    const uint32_t *m_gate;  // their new gate indices (NO_GATE: detach)
    uint32_t n;
    uint32_t G, nb, per;  // gates, blocks, messages per block
    uint32_t *blk_cnt;    // [2][G][nb]: creates then destroys (the scan turns it into bases)
    unsigned long long *sc;  // {create, destroy} records of all blocks (64-bit: the scan's total wraps)
    uint4 *out_c;            // 3 uint4 per create record
    uint4 *out_d;            // 2 uint4 per destroy record
    unsigned long long cap_c, cap_d;  // records they hold (the write pass writes nothing past a larger total)
};

template <bool WRITE>
__device__ __forceinline__ void switch_pass(const SwitchArgs &A) {
    extern __shared__ uint32_t gtab[];  // [2][G] count: the block's records; write: next position of each run
    __shared__ unsigned long long s_tot[2];
    if (WRITE && (A.sc[0] > A.cap_c || A.sc[1] > A.cap_d)) return;  // (as cast_pass: the host regrows and relaunches)
    const uint32_t blk = blockIdx.x, w = threadIdx.x / 64, ln = s_lane();
    for (uint32_t q = threadIdx.x; q < 2 * A.G; q += blockDim.x) gtab[q] = WRITE ? A.blk_cnt[(size_t)q * A.nb + blk] : 0u;
    if (!WRITE && threadIdx.x < 2) s_tot[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t split = WRITE ? A.blk_cnt[(size_t)A.G * A.nb] : 0u;  // destroy bases start here
    const unsigned long long lt = (1ull << ln) - 1ull;
    unsigned long long wtot_c = 0ull, wtot_d = 0ull;  // (wave-uniform)
    const uint32_t m1 = min(A.n, (blk + 1u) * A.per);
    for (uint32_t m = blk * A.per + w; m < m1; m += ST / 64) {
        // the message and the source: its frame index, old gate and old ClientID in one round trip
        const uint32_t slot = rfl(A.m_slot[m]), gnew = rfl(A.m_gate[m]);
        const uint4 cm = A.m_cid[m];
        const uint4 cnew = make_uint4(rfl(cm.x), rfl(cm.y), rfl(cm.z), rfl(cm.w));
        const uint32_t r0 = rfl(A.info.rank[slot]);
        const uint4 st0 = A.slots[SLOT_U4 * (size_t)slot];
        const uint4 co = A.slots[SLOT_U4 * (size_t)slot + 3];
        const uint32_t gold = rfl(st0.x);
        const uint4 cold = make_uint4(rfl(co.x), rfl(co.y), rfl(co.z), rfl(co.w));
        const bool had = gold < A.G, has = gnew < A.G;  // (NO_GATE: no client)
        if (had == has && (!has || (gold == gnew && eq4(cold, cnew)))) continue;  // oldClient == client (Entity.go:680)
        if (r0 >= A.F.n) continue;  // (rank: 0xFFFFFFFF if never live)
        const SlotSp S0 = ld_ss(A.F.ss, r0);
        const Rec16 R = ld_rec(A.F.rec, r0);
        if (rfl(S0.slot) != slot) continue;  // left the frame: nilSpace or a space without AOI, no neighbours
        uint32_t nhit = 0;  // (wave-uniform)
        // a hit's records at its positions: B's EntityID e, slot position record P, frame record fr
        auto put = [&](bool v, uint32_t p_c, uint32_t p_d, const uint4 &e, const uint4 &P, const uint4 &fr) {
            if (v && has && p_c < A.cap_c) {  // x, z of the frame; y, yaw of the slot (k_route's create)
                uint4 *o = A.out_c + 3 * (size_t)p_c;
                o[0] = cnew;
                o[1] = make_uint4(e.x, e.y, e.z, e.w);  // (by component: a whole-vector copy to both records kept the array in scratch)
                o[2] = make_uint4(fr.x, P.y, fr.y, P.w);
            }
            if (v && had && p_d < A.cap_d) {
                uint4 *o = A.out_d + 2 * (size_t)p_d;
                o[0] = cold;
                o[1] = make_uint4(e.x, e.y, e.z, e.w);
            }
        };
        window_walk(A.F, r0, R, S0, w, ln, [&](const uint32_t(&b)[CAST_WU], const uint4(&q)[CAST_WU], const bool(&hit)[CAST_WU]) {
            if (!WRITE) {
#pragma unroll
                for (int u = 0; u < CAST_WU; ++u) nhit += (uint32_t)__popcll(__ballot(hit[u]));
                return;
            }
            // positions: one atomic per table for the step's hits, a hit takes its rank among them
            uint32_t pc[CAST_WU], pd[CAST_WU];
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) {
                const unsigned long long hb = __ballot(hit[u]);
                const uint32_t c = (uint32_t)__popcll(hb), rk = (uint32_t)__popcll(hb & lt);
                uint32_t bc = 0, bd = 0;
                if (ln == 0 && c) {
                    if (has) bc = atomicAdd(&gtab[gnew], c);
                    if (had) bd = atomicAdd(&gtab[A.G + gold], c);
                }
                pc[u] = rfl(bc) + rk;
                pd[u] = rfl(bd) - split + rk;
            }
            // the hits' EntityID and position record; every lane's load is issued (a lane without a
            // hit re-reads the source's)
            uint32_t ds[CAST_WU];
            uint4 ei[CAST_WU], po[CAST_WU];
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) ds[u] = ld_ss(A.F.ss, hit[u] ? b[u] : r0).slot;
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) {
                po[u] = A.slots[SLOT_U4 * (size_t)ds[u] + 1];
                ei[u] = A.slots[SLOT_U4 * (size_t)ds[u] + 2];
            }
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) put(hit[u], pc[u], pd[u], ei[u], po[u], q[u]);
        });
        if (!WRITE && nhit) {
            if (has) wtot_c += nhit;
            if (had) wtot_d += nhit;
            if (ln == 0) {
                if (has) atomicAdd(&gtab[gnew], nhit);
                if (had) atomicAdd(&gtab[A.G + gold], nhit);
            }
        }
    }
    if (WRITE) return;
    if (ln == 0 && wtot_c) atomicAdd(&s_tot[0], wtot_c);
    if (ln == 0 && wtot_d) atomicAdd(&s_tot[1], wtot_d);
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < 2 * A.G; q += blockDim.x) A.blk_cnt[(size_t)q * A.nb + blk] = gtab[q];
    if (threadIdx.x < 2 && s_tot[threadIdx.x]) atomicAdd(&A.sc[threadIdx.x], s_tot[threadIdx.x]);  // two per block
    if (threadIdx.x == 0 && blk == 0) A.blk_cnt[2 * (size_t)A.G * A.nb] = 0u;  // the scan's last entry: the (32-bit) total
}

__global__ __launch_bounds__(ST) void k_switch_count(SwitchArgs A) { switch_pass<false>(A); }
__global__ __launch_bounds__(ST) void k_switch_write(SwitchArgs A) { switch_pass<true>(A); }

// The switch itself, from the uploaded messages: what gwaoi_entity_set_client leaves (a detach
// keeps the ClientID and clears the gate).  The slots of a batch are distinct.
__global__ void k_switch_apply(const uint4 *__restrict__ m_cid, const uint32_t *__restrict__ m_slot,
                               const uint32_t *__restrict__ m_gate, uint32_t n, uint4 *slots) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    const uint32_t s = m_slot[m], g = m_gate[m];
    if (g != NO_GATE) slots[SLOT_U4 * (size_t)s + 3] = m_cid[m];
    reinterpret_cast<uint32_t *>(slots)[SLOT_W * (size_t)s + SST_GATE] = g;
}

// ------------------------------------------------- interest-set reads ------
// InterestedIn as game logic reads it (Monster.AI's loop, Monster.go:49-65; Entity.IsInterestedIn,
// Entity.go:248-251; Avatar.go:281-307's count by type), for a batch of queries on the relation
// of the last flush: the rows themselves (k_rows_*), membership of a pair (k_related) and the
// nearest neighbour that passes a tag filter (k_nearest).  The rows and the nearest are the
// broadcast's shape: one wave per query, a block a contiguous chunk, its waves every fourth one,
// the source's window walked by window_walk; only hits load the candidate's slot (and tag and y),
// the other lanes re-read the source's through a clamped index.  Nothing takes an atomic per hit:
// a row's length is a popcount kept in a register, a hit's position the row's base plus the
// running count plus its rank among the step's hits, so a row's order is that of the walk.
constexpr unsigned long long Q_E_SLOT = 1ull << 62;  // device forms: a query's slot >= max_slots
constexpr unsigned long long Q_TOTAL = Q_E_SLOT - 1ull;
constexpr uint32_t POS_Y = 4 + 1;  // word of y in a slot record (pos = its second uint4)

// The values of loads that every lane issues and only hits use: pinned here, so that the compiler
// cannot sink a step's loads under that step's hit branch (slot_info's idiom, gwaoi_kernels.hip).
template <class T>
__device__ __forceinline__ void keep_loads(T (&v)[CAST_WU]) {
    static_assert(CAST_WU == 2 && sizeof(T) == 4, "two 32-bit values");
    asm volatile("" : "+v"(v[0]), "+v"(v[1]));
}

struct RowsArgs {
    FrameView F;
    SlotTab info;
    const uint32_t *q_slot;  // the queries' slots
    uint32_t n, max_slots;
    uint32_t per;            // queries per block
    uint32_t *cnt;           // n + 1: count pass: row lengths (cnt[n] = 0); scanned in place: the rows' offsets
    unsigned long long *sc;  // items of all rows (64-bit: the scan's total wraps) | Q_E_SLOT
    uint32_t *items;         // write pass
    unsigned long long cap;  // items it holds (the write pass writes nothing past a larger total)
};

template <bool WRITE>
__device__ __forceinline__ void rows_pass(const RowsArgs &A) {
    __shared__ unsigned long long s_tot;
    // queued behind the count pass and the scan (as cast_pass: the host regrows and relaunches)
    if (WRITE && (*A.sc & Q_TOTAL) > A.cap) return;
    const uint32_t blk = blockIdx.x, w = threadIdx.x / 64, ln = s_lane();
    if (!WRITE) {
        if (threadIdx.x == 0) s_tot = 0ull;
        __syncthreads();
    }
    const unsigned long long lt = (1ull << ln) - 1ull;
    unsigned long long wtot = 0ull, werr = 0ull;  // (wave-uniform)
    const uint32_t m1 = min(A.n, (blk + 1u) * A.per);
    for (uint32_t m = blk * A.per + w; m < m1; m += ST / 64) {
        const uint32_t slot = rfl(A.q_slot[m]);
        const uint32_t base = WRITE ? rfl(A.cnt[m]) : 0u;
        uint32_t run = 0;  // hits so far (wave-uniform)
        const bool ok = slot < A.max_slots;  // (device form only: the host form is checked on the host)
        if (!ok) werr |= Q_E_SLOT;
        const uint32_t r0 = ok ? rfl(A.info.rank[slot]) : 0xFFFFFFFFu;  // (rank: 0xFFFFFFFF if never live)
        if (r0 < A.F.n) {
            const SlotSp S0 = ld_ss(A.F.ss, r0);
            const Rec16 R = ld_rec(A.F.rec, r0);
            if (rfl(S0.slot) == slot)  // (else it left the frame: nilSpace or a space without AOI, an empty row)
                window_walk(A.F, r0, R, S0, w, ln, [&](const uint32_t(&b)[CAST_WU], const uint4(&)[CAST_WU], const bool(&hit)[CAST_WU]) {
                    if (!WRITE) {
#pragma unroll
                        for (int u = 0; u < CAST_WU; ++u) run += (uint32_t)__popcll(__ballot(hit[u]));
                        return;
                    }
                    uint32_t ds[CAST_WU], p[CAST_WU];
#pragma unroll
                    for (int u = 0; u < CAST_WU; ++u) ds[u] = ld_ss(A.F.ss, hit[u] ? b[u] : r0).slot;
                    keep_loads(ds);  // (else the later step's load sinks under its hit branch: a round trip each)
#pragma unroll
                    for (int u = 0; u < CAST_WU; ++u) {
                        const unsigned long long hb = __ballot(hit[u]);
                        p[u] = base + run + (uint32_t)__popcll(hb & lt);
                        run += (uint32_t)__popcll(hb);
                    }
#pragma unroll
                    for (int u = 0; u < CAST_WU; ++u)
                        if (hit[u] && p[u] < A.cap) A.items[p[u]] = ds[u];
                });
        }
        if (!WRITE) {
            if (ln == 0) A.cnt[m] = run;  // once per query
            wtot += run;
        }
    }
    if (WRITE) return;
    if (ln == 0 && wtot) atomicAdd(&s_tot, wtot);
    if (ln == 0 && werr) atomicOr(A.sc, werr);  // (one lane per wave that saw a bad query)
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_tot) atomicAdd(A.sc, s_tot);  // one per block
        if (blk == 0) A.cnt[A.n] = 0u;      // the scan's last entry becomes the (32-bit) total
    }
}

__global__ __launch_bounds__(ST) void k_rows_count(RowsArgs A) { rows_pass<false>(A); }
__global__ __launch_bounds__(ST) void k_rows_write(RowsArgs A) { rows_pass<true>(A); }

// a[m].IsInterestedIn(b[m]): one lane per pair, two rank lookups and two frame records through
// clamped indices, no window walk.
struct RelatedArgs {
    FrameView F;
    SlotTab info;
    const uint32_t *qa, *qb;
    uint32_t n, max_slots;
    unsigned long long *sc;  // Q_E_SLOT
    uint8_t *out;
};

__global__ __launch_bounds__(ST) void k_related(RelatedArgs A) {
    const uint32_t i = blockIdx.x * ST + threadIdx.x;
    const uint32_t m = min(i, A.n - 1u);
    const uint32_t a = A.qa[m], b = A.qb[m];
    const bool bad = a >= A.max_slots || b >= A.max_slots;
    const uint32_t ra = A.info.rank[min(a, A.max_slots - 1u)], rb = A.info.rank[min(b, A.max_slots - 1u)];
    bool r = false;
    if (A.F.n) {  // (uniform: an empty frame has no entry 0 to clamp to)
        const uint32_t ia = ra < A.F.n ? ra : 0u, ib = rb < A.F.n ? rb : 0u;
        const SlotSp Sa = ld_ss(A.F.ss, ia), Sb = ld_ss(A.F.ss, ib);
        const Rec16 Ra = ld_rec(A.F.rec, ia), Rb = ld_rec(A.F.rec, ib);
        const float D = A.F.grid[Sa.sp].D;  // (a frame entry's space: valid whether or not it is a's)
        const bool in = !bad && ra < A.F.n && rb < A.F.n && Sa.slot == a && Sb.slot == b && Sa.sp == Sb.sp && a != b;
        r = in && rel(Ra.x, Ra.z, Ra.s, Rb.x, Rb.z, Rb.s, D);
    }
    if (i < A.n) {
        A.out[i] = r ? 1 : 0;
        if (bad) atomicOr(A.sc, Q_E_SLOT);  // (device form only)
    }
}

// The neighbour b of each query's source with (tag[b] & mask) == want and the smallest
// (squared distance, slot): one wave per query, the rows' walk.  A hit loads its slot, then its
// tag and y; each lane keeps the smallest key (d2 bits << 32) | slot (d2 >= 0: its bits order as
// unsigned), a wave min-reduction combines them and lane 0 stores the query's 8 B.
struct NearArgs {
    FrameView F;
    SlotTab info;
    const uint4 *slots;   // SLOT_U4 per slot (y)
    const uint32_t *tag;  // per slot
    const uint32_t *q_slot, *q_mask, *q_want;  // (q_mask nullptr: every neighbour passes)
    uint32_t n, max_slots;
    uint32_t per;  // queries per block
    unsigned long long *sc;  // Q_E_SLOT
    uint32_t *out_slot;
    float *out_dist;
};

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        v = min(v, ((unsigned long long)hi << 32) | lo);
    }
    return v;
}

__global__ __launch_bounds__(ST) void k_nearest(NearArgs A) {
    const uint32_t blk = blockIdx.x, w = threadIdx.x / 64, ln = s_lane();
    const float *sw = reinterpret_cast<const float *>(A.slots);
    unsigned long long werr = 0ull;  // (wave-uniform)
    const uint32_t m1 = min(A.n, (blk + 1u) * A.per);
    for (uint32_t m = blk * A.per + w; m < m1; m += ST / 64) {
        const uint32_t slot = rfl(A.q_slot[m]);
        const uint32_t mask = A.q_mask ? rfl(A.q_mask[m]) : 0u, want = A.q_mask ? rfl(A.q_want[m]) : 0u;
        unsigned long long best = ~0ull;
        const bool ok = slot < A.max_slots;
        if (!ok) werr |= Q_E_SLOT;
        const uint32_t r0 = ok ? rfl(A.info.rank[slot]) : 0xFFFFFFFFu;
        if (r0 < A.F.n) {
            const SlotSp S0 = ld_ss(A.F.ss, r0);
            const Rec16 R = ld_rec(A.F.rec, r0);
            const float y0 = sw[SLOT_W * (size_t)slot + POS_Y];
            if (rfl(S0.slot) == slot)
                window_walk(A.F, r0, R, S0, w, ln, [&](const uint32_t(&b)[CAST_WU], const uint4(&q)[CAST_WU], const bool(&hit)[CAST_WU]) {
                    uint32_t ds[CAST_WU], tg[CAST_WU];
                    float y[CAST_WU];
#pragma unroll
                    for (int u = 0; u < CAST_WU; ++u) ds[u] = ld_ss(A.F.ss, hit[u] ? b[u] : r0).slot;
#pragma unroll
                    for (int u = 0; u < CAST_WU; ++u) {
                        tg[u] = A.tag[ds[u]];
                        y[u] = sw[SLOT_W * (size_t)ds[u] + POS_Y];
                    }
                    keep_loads(tg);  // (issued together for both steps, not under the later step's hit branch)
                    keep_loads(y);
#pragma unroll
                    for (int u = 0; u < CAST_WU; ++u) {
                        // Vector3.DistanceTo's sum (Vector3.go:22-28), float32 step by step (no contraction)
                        const float dx = __uint_as_float(q[u].x) - R.x, dy = y[u] - y0, dz = __uint_as_float(q[u].y) - R.z;
                        const float d2 = (dx * dx + dy * dy) + dz * dz;
                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | ds[u];
                        if (hit[u] && (tg[u] & mask) == want) best = min(best, key);
                    }
                });
        }
        best = wave_min_u64(best);
        if (ln == 0) {
            const bool none = best == ~0ull;
            A.out_slot[m] = none ? GWAOI_NO_SLOT : (uint32_t)best;
            A.out_dist[m] = none ? __uint_as_float(0x7F800000u) : (float)sqrt((double)__uint_as_float((uint32_t)(best >> 32)));
        }
    }
    if (ln == 0 && werr) atomicOr(A.sc, werr);
}

// ------------------------------------------------------- range reads ------
// The entities within a caller-chosen radius of an entity or of a point (gwaoi_range_batch): the
// rows' shape (one wave per query, count / scan / write, no atomic per hit) over a window that is
// not the go-aoi window and a centre that need not be a frame entry.  The window is centre -+
// radius in the grid of the query's space, widened by range_window's margin (gwaoi_range.h;
// it holds every hit), and may have any number of grid rows.  A candidate is tested
// in two steps: the distance without dy from its frame record alone (never larger than the full
// one, and the full one with GWAOI_RANGE_PLANAR), then only those lanes go on to the candidate's
// slot, tag and y; the others re-read entry `clamp` (the centre's own, or entry 0 for a point).
constexpr unsigned long long Q_E_INVAL = 1ull << 61;      // device forms: a flag bit outside the two, radius < 0
constexpr unsigned long long Q_E_NONFINITE = 1ull << 60;  // device forms: a radius or point coordinate NaN or infinite
constexpr unsigned long long Q_E_SPACE = 1ull << 59;      // device forms: a point's space id >= max_spaces
constexpr unsigned long long RANGE_TOTAL = Q_E_SPACE - 1ull;
constexpr uint32_t RANGE_NO_SELF = 0xFFFFFFFFu;  // a point query excludes nobody

__device__ __forceinline__ float rflf(float v) { return __uint_as_float(rfl(__float_as_uint(v))); }

// window_walk's walk over the cell rectangle W of grid gr: lane j loads row j's bounds, 64 rows at a
// time, the rows are laid end to end and the wave reads 64 consecutive candidates per step, CAST_WU
// steps with their loads in flight together.  step(b, q, live): lane ln's candidate of step u is
// frame index b[u] with frame record q[u]; a lane past the window's end has live[u] false and
// b[u] == clamp, a valid frame index (the frame is not empty).  The row layout (s_adj, s_mark) is
// window_walk's, kept apart so that its users' code stays as it is: a fix to that scheme goes into both.
template <class Step>
__device__ __forceinline__ void range_walk(const FrameView &F, const SpaceGrid &gr, const RangeWindow &W, uint32_t clamp,
                                           uint32_t w, uint32_t ln, Step &&step) {
    __shared__ uint32_t s_adj[ST / 64][64];             // candidate index - position, per non-empty row
    __shared__ uint32_t s_mark[ST / 64][CAST_WU * 64];  // a non-empty row starts at this position
    const uint32_t *cs = F.cell_start;
    const uint4 *frec = reinterpret_cast<const uint4 *>(F.rec);
    const unsigned long long lt = (1ull << ln) - 1ull;
    const unsigned long long le = ln == 63 ? ~0ull : (2ull << ln) - 1ull;
    const uint32_t span = rfl((uint32_t)(W.cx1 - W.cx0) + 1u), nrows = rfl((uint32_t)(W.cz1 - W.cz0) + 1u);
    const uint32_t row0 = rfl(gr.base + (uint32_t)W.cz0 * gr.gx + (uint32_t)W.cx0), gx = rfl(gr.gx);
    for (uint32_t j0 = 0; j0 < nrows; j0 += 64u) {
        // lane t: row j0 + t of the window, its candidates [jb, je)
        const uint32_t t = j0 + ln;
        const uint32_t rb = row0 + min(t, nrows - 1u) * gx;
        const uint32_t jb = cs[rb], je = cs[rb + span];
        const uint32_t len = t < nrows ? je - jb : 0u;
        const uint32_t incl = wave_scan_add(len);
        const uint32_t ex = incl - len, T = rdl(incl, 63);
        const unsigned long long nem = __ballot(len != 0u);
        if (len) s_adj[w][__popcll(nem & lt)] = jb - ex;
        for (uint32_t p0 = 0; p0 < T; p0 += CAST_WU * 64u) {
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) s_mark[w][u * 64 + ln] = 0u;
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            if (len && ex >= p0 && ex - p0 < CAST_WU * 64u) s_mark[w][ex - p0] = 1u;
            uint32_t nr = (uint32_t)__popcll(__ballot(len != 0u && ex < p0));  // non-empty rows started before this step
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            uint32_t b[CAST_WU];
            uint4 q[CAST_WU];
            bool live[CAST_WU];
#pragma unroll
            for (int u = 0; u < CAST_WU; ++u) {
                const unsigned long long mk = __ballot(s_mark[w][u * 64 + ln] != 0u);
                const uint32_t p = p0 + (uint32_t)u * 64u + ln;
                const uint32_t row = nr + (uint32_t)__popcll(mk & le);  // rows started at or before p
                nr += (uint32_t)__popcll(mk);
                live[u] = p < T;
                b[u] = live[u] ? p + s_adj[w][row - 1u] : clamp;  // (row >= 1 whenever p < T)
                q[u] = frec[b[u]];
            }
            step(b, q, live);
        }
        __builtin_amdgcn_wave_barrier();  // s_adj is rewritten by the next row group
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
}

struct RangeArgs {
    FrameView F;
    SlotTab info;
    const uint4 *slots;   // SLOT_U4 per slot (y)
    const uint32_t *tag;  // per slot
    const uint4 *q;       // two per query (gwaoi_range_query)
    uint32_t n, max_slots, max_spaces;
    uint32_t n_grids;     // entries of F.grid (a space created after the flush has none: an empty row)
    uint32_t per;         // queries per block
    uint32_t scan;        // cnt has n + 1 entries and is scanned next (else: the count form's n answers)
    uint32_t *cnt;        // count pass: row lengths (cnt[n] = 0); scanned in place: the rows' offsets
    unsigned long long *sc;  // items of all rows | Q_E_*
    uint32_t *items;         // write pass
    float *dists;            // parallel to items
    unsigned long long cap;  // items either holds (the write pass writes nothing past a larger total)
};

template <bool WRITE>
__device__ __forceinline__ void range_pass(const RangeArgs &A) {
    __shared__ unsigned long long s_tot;
    // queued behind the count pass and the scan (as rows_pass: the host regrows and relaunches)
    if (WRITE && (*A.sc & RANGE_TOTAL) > A.cap) return;
    const uint32_t blk = blockIdx.x, w = threadIdx.x / 64, ln = s_lane();
    if (!WRITE) {
        if (threadIdx.x == 0) s_tot = 0ull;
        __syncthreads();
    }
    const float *sw = reinterpret_cast<const float *>(A.slots);
    const unsigned long long lt = (1ull << ln) - 1ull;
    unsigned long long wtot = 0ull, werr = 0ull;  // (wave-uniform)
    const uint32_t m1 = min(A.n, (blk + 1u) * A.per);
    for (uint32_t m = blk * A.per + w; m < m1; m += ST / 64) {
        // the query record: one 32-B load per wave
        const uint4 qa = A.q[2 * (size_t)m], qb = A.q[2 * (size_t)m + 1];
        const uint32_t center = rfl(qa.x), fl = rfl(qa.y), mask = rfl(qb.z), want = rfl(qb.w);
        const float px = __uint_as_float(rfl(qa.z)), py = __uint_as_float(rfl(qa.w)), pz = __uint_as_float(rfl(qb.x));
        const float rad = __uint_as_float(rfl(qb.y));
        const uint32_t base = WRITE ? rfl(A.cnt[m]) : 0u;
        uint32_t run = 0;  // hits so far (wave-uniform)
        const bool point = fl & GWAOI_RANGE_POINT, planar = fl & GWAOI_RANGE_PLANAR;
        const float inf = __uint_as_float(0x7F800000u);
        // (device forms only: the host forms are checked on the host)
        unsigned long long e = 0ull;
        if (fl & ~(GWAOI_RANGE_POINT | GWAOI_RANGE_PLANAR)) e |= Q_E_INVAL;
        if (!(fabsf(rad) < inf)) e |= Q_E_NONFINITE;
        else if (rad < 0.0f) e |= Q_E_INVAL;  // (-0.0 is 0)
        if (point) {
            if (!(fabsf(px) < inf && fabsf(py) < inf && fabsf(pz) < inf)) e |= Q_E_NONFINITE;
            if (center >= A.max_spaces) e |= Q_E_SPACE;
        } else if (center >= A.max_slots) {
            e |= Q_E_SLOT;
        }
        werr |= e;
        // the centre, its space and the entry idle lanes re-read; an empty frame has no entry at all
        bool go = !e && A.F.n != 0u;
        uint32_t sp = 0u, self = RANGE_NO_SELF, clamp = 0u;
        float cx = px, cy = py, cz = pz;
        if (go && point) {
            sp = center;
            go = sp < A.n_grids;
        } else if (go) {
            const uint32_t r0 = rfl(A.info.rank[center]);  // (rank: 0xFFFFFFFF if never live)
            go = r0 < A.F.n;
            if (go) {
                const SlotSp S0 = ld_ss(A.F.ss, r0);
                const Rec16 R = ld_rec(A.F.rec, r0);
                go = rfl(S0.slot) == center;  // (else it left the frame: nilSpace or a space without AOI)
                sp = rfl(S0.sp);
                cx = rflf(R.x);
                cz = rflf(R.z);
                cy = rflf(sw[SLOT_W * (size_t)center + POS_Y]);
                self = clamp = r0;
            }
        }
        if (go) {
            const SpaceGrid gr = A.F.grid[sp];
            const RangeWindow W = range_window(cx, cz, rad, gr.ox, gr.oz, gr.inv, gr.gx, gr.gz);
            range_walk(A.F, gr, W, clamp, w, ln, [&](const uint32_t(&b)[CAST_WU], const uint4(&q)[CAST_WU], const bool(&live)[CAST_WU]) {
                bool pre[CAST_WU];
                uint32_t ds[CAST_WU], tg[CAST_WU];
                float y[CAST_WU], dp[CAST_WU];
#pragma unroll
                for (int u = 0; u < CAST_WU; ++u) {
                    // without dy: fl(fl(a + b) + c) >= fl(a + c) for b >= 0, so no hit fails this
                    const float dx = __uint_as_float(q[u].x) - cx, dz = __uint_as_float(q[u].y) - cz;
                    dp[u] = range_dist(range_d2(dx, 0.0f, dz, true));
                }
                keep_loads(dp);  // (both steps' square roots, then both slot loads: no branch around either)
#pragma unroll
                for (int u = 0; u < CAST_WU; ++u) {
                    pre[u] = live[u] && b[u] != self && dp[u] <= rad;
                    ds[u] = ld_ss(A.F.ss, pre[u] ? b[u] : clamp).slot;
                }
#pragma unroll
                for (int u = 0; u < CAST_WU; ++u) {
                    tg[u] = A.tag[ds[u]];
                    y[u] = sw[SLOT_W * (size_t)ds[u] + POS_Y];
                }
                keep_loads(tg);  // (issued together for both steps, not under the later step's hit branch)
                keep_loads(y);
#pragma unroll
                for (int u = 0; u < CAST_WU; ++u) {
                    float dist;
                    const bool in = range_hit(cx, cy, cz, __uint_as_float(q[u].x), y[u], __uint_as_float(q[u].y), planar, rad, &dist);
                    const bool hit = pre[u] && in && (tg[u] & mask) == want;
                    const unsigned long long hb = __ballot(hit);
                    const uint32_t p = base + run + (uint32_t)__popcll(hb & lt);
                    run += (uint32_t)__popcll(hb);
                    if (WRITE && hit && p < A.cap) {
                        A.items[p] = ds[u];
                        A.dists[p] = dist;
                    }
                }
            });
        }
        if (!WRITE) {
            if (ln == 0) A.cnt[m] = run;  // once per query
            wtot += run;
        }
    }
    if (WRITE) return;
    if (ln == 0 && wtot) atomicAdd(&s_tot, wtot);
    if (ln == 0 && werr) atomicOr(A.sc, werr);  // (one lane per wave that saw a bad query)
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_tot) atomicAdd(A.sc, s_tot);         // one per block
        if (blk == 0 && A.scan) A.cnt[A.n] = 0u;  // the scan's last entry becomes the (32-bit) total
    }
}

__global__ __launch_bounds__(ST) void k_range_count(RangeArgs A) { range_pass<false>(A); }
__global__ __launch_bounds__(ST) void k_range_write(RangeArgs A) { range_pass<true>(A); }

// ------------------------------------------------ server-driven movement ------
// Monster.Tick's chase and FaceTo (Monster.go:80-102, Entity.go:1292-1304, Vector3.go:44-77) for a
// batch of (mover, target, step, flags) messages: one lane per message, k_related's gate (two rank
// lookups, two frame records, one rel()) and then a handful of float32 operations in the reference's
// order.  Compute-then-apply: k_steer reads the frame and the movers' slot records, which nothing in
// it writes, and leaves each applied message's result in the outputs, its Moved op in the batch
// arrays and its claim in cl; k_steer_apply then writes the slot records of the messages whose claim
// store survived (the decode's claim-store-then-compare: a mover named twice keeps one message).
constexpr uint32_t STEER_E_SLOT = 1u, STEER_E_INVAL = 2u, STEER_E_NONFINITE = 4u;  // the status word
constexpr uint32_t STEER_ALL = GWAOI_STEER_MOVE | GWAOI_STEER_FACE;

struct SteerArgs {
    FrameView F;
    SlotTab info;
    const uint4 *slots;  // SLOT_U4 per slot: sst, pos, eid, cid
    const uint32_t *mv, *tg;
    const float *step;
    const uint32_t *flags;  // nullptr: MOVE | FACE for every message
    uint32_t n, max_slots;
    uint32_t *o_slot, *o_sp;  // the device Moved batch (SLOT_NONE: no move)
    float *o_x, *o_z;
    uint32_t *o_ms;  // mover of an applied message (SLOT_NONE: not applied), for k_steer_apply
    unsigned long long claim0;
    unsigned long long *cl;
    uint32_t *sst;
    float4 *pos;
    uint8_t *out_applied;
    float *out_pos;  // 4 per message: x, y, z, yaw
    uint32_t *status;  // STEER_E_*
};

// Vector3.Normalize as written (Vector3.go:64-72): the sum takes Y itself, twice, not its square.
__device__ __forceinline__ void steer_normalize(float &x, float &y, float &z) {
    const float sum = ((x * x + y) + y) + z * z;
    const float d = (float)sqrt((double)sum);
    if (d == 0.0f) return;
    x = x / d;
    y = y / d;
    z = z / d;
}

// Vector3.DirToYaw (Vector3.go:45-62) of a direction with Y = 0: float64 throughout, then Yaw(float32).
__device__ __forceinline__ float steer_dir_to_yaw(float x, float z) {
    float y = 0.0f;
    steer_normalize(x, y, z);
    double yaw = acos((double)x);
    if (z < 0.0f) yaw = 6.283185307179586 - yaw;
    yaw = yaw / 3.141592653589793 * 180.0;
    yaw = yaw <= 90.0 ? 90.0 - yaw : 90.0 + (360.0 - yaw);
    return (float)yaw;
}

__global__ __launch_bounds__(ST) void k_steer(SteerArgs A) {
    const uint32_t i = blockIdx.x * ST + threadIdx.x;
    const uint32_t m = min(i, A.n - 1u);
    const uint32_t a = A.mv[m], b = A.tg[m];
    const float s = A.step[m];
    const uint32_t fl = A.flags ? A.flags[m] : STEER_ALL;
    uint32_t err = 0;  // (device form only: the host form is checked on the host)
    if (a >= A.max_slots || (b >= A.max_slots && b != GWAOI_NO_SLOT)) err |= STEER_E_SLOT;
    if (fl & ~STEER_ALL) err |= STEER_E_INVAL;
    if (!(fabsf(s) <= 3.402823466e+38f)) err |= STEER_E_NONFINITE;
    // every load through a clamped index, none under a per-lane branch: the two ranks and the mover's
    // record in one round trip, the two frame entries and records in the next
    const uint32_t ac = min(a, A.max_slots - 1u), bc = min(b, A.max_slots - 1u);
    uint32_t ra = A.info.rank[ac], rb = A.info.rank[bc];
    uint32_t sp = reinterpret_cast<const uint32_t *>(A.slots)[SLOT_W * (size_t)ac + SST_SPACE];
    float y = reinterpret_cast<const float *>(A.slots)[SLOT_W * (size_t)ac + POS_Y];
    float yaw = reinterpret_cast<const float *>(A.slots)[SLOT_W * (size_t)ac + POS_Y + 2];
    asm volatile("" : "+v"(ra), "+v"(rb), "+v"(sp), "+v"(y), "+v"(yaw));  // (issued together, none sunk under a branch)
    bool on = false;
    float x = 0.f, z = 0.f;
    if (A.F.n) {  // (uniform: an empty frame has no entry 0 to clamp to)
        const uint32_t ia = ra < A.F.n ? ra : 0u, ib = rb < A.F.n ? rb : 0u;
        SlotSp Sa = ld_ss(A.F.ss, ia), Sb = ld_ss(A.F.ss, ib);
        Rec16 Ra = ld_rec(A.F.rec, ia), Rb = ld_rec(A.F.rec, ib);
        // (else the gate's && chain loads the seqs, and D, only in the lanes that got that far)
        asm volatile("" : "+v"(Sa.slot), "+v"(Sa.sp), "+v"(Sb.slot), "+v"(Sb.sp), "+v"(Ra.x), "+v"(Ra.z), "+v"(Ra.s),
                     "+v"(Rb.x), "+v"(Rb.z), "+v"(Rb.s));
        float D = A.F.grid[Sa.sp].D;  // (a frame entry's space: valid whether or not it is the mover's)
        asm volatile("" : "+v"(D));
        // mover.IsInterestedIn(target), as k_related answers it (GWAOI_NO_SLOT is not in the frame)
        on = !err && fl != 0u && b < A.max_slots && ra < A.F.n && rb < A.F.n && Sa.slot == a && Sb.slot == b &&
             Sa.sp == Sb.sp && a != b && rel(Ra.x, Ra.z, Ra.s, Rb.x, Rb.z, Rb.s, D);
        x = Ra.x;
        z = Ra.z;
        if (fl & GWAOI_STEER_MOVE) {  // mypos + Normalized(target - mypos, Y = 0) * step
            float dx = Rb.x - x, dy = 0.0f, dz = Rb.z - z;
            steer_normalize(dx, dy, dz);
            x = x + dx * s;
            y = y + dy * s;
            z = z + dz * s;
        }
        if (fl & GWAOI_STEER_FACE) yaw = steer_dir_to_yaw(Rb.x - x, Rb.z - z);  // (from the new position)
    }
    if (i >= A.n) return;
    // a Position the flush would refuse never reaches the slot record
    if (on && !(fabsf(x) <= 3.402823466e+38f && fabsf(z) <= 3.402823466e+38f && yaw == yaw)) {
        on = false;
        err |= STEER_E_NONFINITE;
    }
    A.o_slot[i] = on && (fl & GWAOI_STEER_MOVE) ? a : SLOT_NONE;
    A.o_x[i] = x;
    A.o_z[i] = z;
    A.o_sp[i] = sp;  // SST_SPACE (no op is queued: the frame's)
    A.o_ms[i] = on ? a : SLOT_NONE;
    A.out_applied[i] = on ? 1 : 0;
    float *o = A.out_pos + 4 * (size_t)i;
    o[0] = on ? x : 0.f;
    o[1] = on ? y : 0.f;
    o[2] = on ? z : 0.f;
    o[3] = on ? yaw : 0.f;
    if (on) {
        // a plain store, as the decode's: this call's claims are larger than every claim applied so
        // far.  Both words whatever the flags: the Position word doubles as the repeated-mover check.
        const unsigned long long c = A.claim0 + i;
        reinterpret_cast<ulonglong2 *>(A.cl)[a] = make_ulonglong2(c, c);
    }
    if (err) atomicOr(A.status, err);  // (rare: a dropped message)
}

// The survivors of the claim compare write their slot records: Position for MOVE, yaw for FACE, and
// both sync flags.  A message whose store was overwritten by another message of the same mover is
// dropped and reported.
__global__ __launch_bounds__(ST) void k_steer_apply(SteerArgs A) {
    const uint32_t i = blockIdx.x * ST + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t s = A.o_ms[i];
    if (s == SLOT_NONE) return;
    float *o = A.out_pos + 4 * (size_t)i;
    if (A.cl[2 * (size_t)s] != A.claim0 + i) {
        A.o_slot[i] = SLOT_NONE;
        A.out_applied[i] = 0;
        o[0] = o[1] = o[2] = o[3] = 0.f;
        atomicOr(A.status, STEER_E_INVAL);
        return;
    }
    const uint32_t fl = A.flags ? A.flags[i] : STEER_ALL;
    float *p = reinterpret_cast<float *>(A.pos + SLOT_U4 * (size_t)s);
    if (fl & GWAOI_STEER_MOVE) {
        p[0] = o[0];
        p[1] = o[1];
        p[2] = o[2];
    }
    if (fl & GWAOI_STEER_FACE) p[3] = o[3];
    uint32_t *f = A.sst + SLOT_W * (size_t)s + SST_FLAGS;
    *f = *f | SIDE_SIF;
}

// -------------------------------------------------------------- route ------
struct RouteArgs {
    const uint32_t *ev;  // (a,b) pairs: [enters | leaves]
    uint32_t n_enter, n_total;
    FrameView F;
    SlotTab info;
    const uint4 *eid, *cid;
    const uint32_t *sst;
    const float4 *pos;
    uint32_t G, nb;
    uint32_t *blk_cnt;  // [2][G][nb]: creates then destroys
    uint4 *out_c;       // 3 uint4 per create record
    uint4 *out_d;       // 2 uint4 per destroy record
    uint32_t split;     // destroy bases start at split (one scan over both parts)
};

template <int PASS>
__global__ __launch_bounds__(ST) void k_route(RouteArgs A) {
    extern __shared__ uint32_t lds[];  // [2][G]
    const uint32_t blk = blockIdx.x;
    for (uint32_t g = threadIdx.x; g < 2 * A.G; g += blockDim.x)
        lds[g] = PASS == 0 ? 0u : A.blk_cnt[(size_t)g * A.nb + blk];
    __syncthreads();
    const uint32_t e = blk * ST + threadIdx.x;
    if (e < A.n_total) {
        const uint2 ab = reinterpret_cast<const uint2 *>(A.ev)[e];
        const uint32_t g = A.sst[SLOT_W * (size_t)ab.x + SST_GATE];
        if (g != NO_GATE) {
            const bool create = e < A.n_enter;
            const uint32_t p = atomicAdd(&lds[(create ? 0u : A.G) + g], 1u);
            if (PASS == 1) {
                if (create) {
                    const uint32_t r = A.info.rank[ab.y];  // b is live after the flush
                    const Rec16 B = ld_rec(A.F.rec, r);
                    const float4 P = A.pos[SLOT_U4 * (size_t)ab.y];
                    uint4 *o = A.out_c + 3 * (size_t)p;
                    o[0] = A.cid[SLOT_U4 * (size_t)ab.x];
                    o[1] = A.eid[SLOT_U4 * (size_t)ab.y];
                    o[2] = make_uint4(__float_as_uint(B.x), __float_as_uint(P.y), __float_as_uint(B.z),
                                      __float_as_uint(P.w));
                } else {
                    uint4 *o = A.out_d + 2 * (size_t)(p - A.split);
                    o[0] = A.cid[SLOT_U4 * (size_t)ab.x];
                    o[1] = A.eid[SLOT_U4 * (size_t)ab.y];
                }
            }
        }
    }
    __syncthreads();
    if (PASS == 0)
        for (uint32_t g = threadIdx.x; g < 2 * A.G; g += blockDim.x) A.blk_cnt[(size_t)g * A.nb + blk] = lds[g];
}

// offsets[k] = scanned[k * nb] for k in [0, parts]; scanned has parts*nb + 1 entries
__global__ void k_part_offsets(const uint32_t *__restrict__ scanned, uint32_t parts, uint32_t nb,
                               unsigned long long *off, const unsigned long long *extra) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= parts) off[k] = scanned[(size_t)k * nb];
    if (k == parts) off[parts + 1] = extra ? *extra : 0ull;  // (one copy brings both to the host)
}

}  // namespace

// ======================================================== host state ======

struct SyncState {
    gwaoi_world *w = nullptr;
    hipStream_t st = nullptr;  // view: the world's stream
    uint32_t max_slots = 0;
    // device, per slot
    DevBuf<uint4> slots;   // SLOT_U4 per slot (the allocation); the four views below point into it
    uint4 *eid = nullptr, *cid = nullptr;
    uint32_t *sst = nullptr;  // gate, space, syncing, flags
    float4 *pos = nullptr;
    DevBuf<uint32_t> tag;  // 32 caller-defined bits per slot (gwaoi_entity_set_tag): an array of its own
    DevBuf<unsigned long long> cl;  // 2 per slot: Position / yaw last-writer claims
    DevBuf<uint32_t> oflag, oflag_n;  // decode: slots flagged outside every AOI space
    uint32_t oflag_cap = 0;           // entries of oflag (max_slots)
    bool decoded = false;             // a decode ran since the last collect
    PinnedBuf<uint32_t> h_ndec;       // oflag_n after the last decode
    Event ndec_ev;                    // that copy
    // id -> slot hash table (device, host mirror)
    DevBuf<uint4> htab;  // 4 per bucket: 3 keys, (slot, slot, slot, -)
    uint32_t hcap = 0, hused = 0;  // entries (3 per 64-B bucket), live + tombstones
    uint32_t hbuckets = 0;         // power of two
    std::vector<uint4> h_hkey;
    std::vector<uint32_t> h_hval;
    std::vector<uint4> h_tab;  // rehash upload staging
    // host mirrors
    std::vector<uint4> h_eid;
    std::vector<uint8_t> h_bound, h_client;
    std::vector<uint8_t> h_plain;  // in a space without AOI (gwaoi_entity_enter_plain)
    std::vector<uint32_t> h_bucket;  // slot -> its hash bucket (if bound)
    std::unordered_map<uint32_t, uint32_t> gate_idx;  // gate id -> dense index
    std::vector<uint16_t> gate_ids;
    // pending device writes
    std::vector<W32> w32;
    std::vector<W128> w128;
    std::vector<SideOp> side;
    std::vector<uint32_t> left;  // slots flagged outside the frame since the last collect (host ops)
    unsigned long long claim_next = 1;
    // staging (pinned host + device), reused once the previous upload has landed
    PinnedBuf<char> h_stage;  // the two grow together, d_stage last (its capacity is the pair's)
    DevBuf<char> d_stage;
    Event stage_ev;
    bool stage_pending = false;
    // decode arenas: alive until the flush that consumes them
    struct Chunk {
        DevBuf<char> buf;
        size_t used;
    };
    std::vector<Chunk> arena;
    uint64_t arena_tick = ~0ull;
    // collect scratch / outputs
    DevBuf<uint32_t> blk_cnt, scan_tmp;
    DevBuf<unsigned long long> d_off;
    PinnedBuf<uint8_t> h_offp;  // d_off (and the extra word) on the host
    DevBuf<uint32_t> d_left;
    // fan-out scratch, frame order: the seven grow together (f_rec: 2 per entry)
    DevBuf<uint32_t> f_snd, f_rg, f_cnt, f_sb;
    DevBuf<uint4> f_rec, f_frec, f_cid;
    DevBuf<uint32_t> scr;  // fan-out hits (sender entries), receiver runs
    DevBuf<unsigned long long> scr_cursor;
    DevBuf<uint4> out, out_d;
    std::vector<unsigned long long> h_off_raw;
    std::vector<uint64_t> h_off, h_off_c, h_off_d;
    PinnedBuf<uint8_t> h_rec, h_rec_d;
    // broadcast collect: the host form's uploaded messages, the total / error word, and outputs
    // of its own (valid until the next broadcast collect, whatever the other collects do)
    DevBuf<uint32_t> cast_in;
    DevBuf<unsigned long long> cast_sc;
    DevBuf<uint4> cast_out;
    PinnedBuf<uint8_t> h_cast;
    std::vector<uint64_t> h_off_cast;
    // client-switch collect: the 64-bit totals {creates, destroys}, outputs of its own (valid until
    // the next switch collect) and a per-slot stamp that finds a slot named twice in one batch
    DevBuf<unsigned long long> sw_sc;
    PinnedBuf<unsigned long long> h_sw_sc;
    DevBuf<uint4> sw_out_c, sw_out_d;
    PinnedBuf<uint8_t> h_sw_c, h_sw_d;
    std::vector<uint64_t> h_off_swc, h_off_swd;
    std::vector<uint32_t> sw_stamp, sw_gate;  // sw_gate: the batch's new gate indices
    uint32_t sw_epoch = 0;
    PinnedBuf<uint32_t> h_steer;  // gwaoi_steer_batch: the status word on the host
};

namespace {

enum Arr { A_CGATE, A_QSPACE, A_SYNCING, A_SFLAGS, A_HVAL, A_TAG, A_N32 };
enum Arr128 { B_EID, B_CID, B_HKEY, B_N128 };

ArrTable table32(SyncState *S) {
    ArrTable T{};
    T.p[A_CGATE] = S->sst + SST_GATE;
    T.p[A_QSPACE] = S->sst + SST_SPACE;
    T.p[A_SYNCING] = S->sst + SST_SYNCING;
    T.p[A_SFLAGS] = S->sst + SST_FLAGS;
    for (int a = A_CGATE; a <= A_SFLAGS; ++a) T.stride[a] = SLOT_W;
    T.p[A_HVAL] = reinterpret_cast<uint32_t *>(S->htab.get());  // index: the slot word of an entry (hval_word)
    T.stride[A_HVAL] = 1;
    T.p[A_TAG] = S->tag.get();
    T.stride[A_TAG] = 1;
    return T;
}
ArrTable table128(SyncState *S) {
    ArrTable T{};
    T.p[B_EID] = S->eid;
    T.stride[B_EID] = SLOT_U4;
    T.p[B_CID] = S->cid;
    T.stride[B_CID] = SLOT_U4;
    T.p[B_HKEY] = S->htab;  // index: the key of an entry (hkey_vec)
    T.stride[B_HKEY] = 1;
    return T;
}

void put32(SyncState *S, Arr a, uint32_t idx, uint32_t v) { S->w32.push_back(W32{(uint32_t)a, idx, v, 0}); }
void put128(SyncState *S, Arr128 a, uint32_t idx, uint4 v) { S->w128.push_back(W128{(uint32_t)a, idx, 0, 0, v}); }

int ensure_stage(SyncState *S, size_t bytes) {
    if (S->stage_pending) {
        HIP_TRY(S->w, hipEventSynchronize(S->stage_ev));
        S->stage_pending = false;
    }
    if (bytes <= S->d_stage.cap()) return GWAOI_OK;
    const size_t cap = std::max<size_t>(bytes + bytes / 2, 1 << 16);
    S->d_stage.reset();
    int rc = alloc_pinned(S->w, S->h_stage, cap);
    if (!rc && (rc = alloc_all(S->w, S->d_stage, cap))) S->h_stage.reset();
    return rc;
}

// Keep the last write per (array, index): one scatter launch has no order.
template <class T>
void last_wins(std::vector<T> &v) {
    if (v.size() < 2) return;
    std::vector<uint32_t> ord(v.size());
    for (uint32_t i = 0; i < ord.size(); ++i) ord[i] = i;
    auto key = [&](uint32_t i) { return ((unsigned long long)v[i].arr << 32) | v[i].idx; };
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    std::vector<T> out;
    out.reserve(v.size());
    for (size_t k = 0; k < ord.size(); ++k)
        if (k + 1 == ord.size() || key(ord[k + 1]) != key(ord[k])) out.push_back(v[ord[k]]);
    v.swap(out);
}

// Upload the pending host-side writes and Y/yaw ops (stream order).
int push(SyncState *S) {
    last_wins(S->w32);
    last_wins(S->w128);
    const size_t b32 = S->w32.size() * sizeof(W32), b128 = S->w128.size() * sizeof(W128);
    const size_t bside = S->side.size() * sizeof(SideOp);
    const size_t total = b128 + b32 + bside;
    if (!total) return GWAOI_OK;
    if (int rc = ensure_stage(S, total)) return rc;
    char *h = S->h_stage, *d = S->d_stage;
    std::memcpy(h, S->w128.data(), b128);
    std::memcpy(h + b128, S->w32.data(), b32);
    std::memcpy(h + b128 + b32, S->side.data(), bside);
    HIP_TRY(S->w, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, S->st));
    HIP_TRY(S->w, hipEventRecord(S->stage_ev, S->st));
    S->stage_pending = true;
    // 128-bit writes first (hash keys before the values that publish them)
    if (!S->w128.empty())
        k_scatter128<<<cdivu(S->w128.size(), ST), ST, 0, S->st>>>(reinterpret_cast<const W128 *>(d),
                                                                   (uint32_t)S->w128.size(), table128(S));
    if (!S->w32.empty())
        k_scatter32<<<cdivu(S->w32.size(), ST), ST, 0, S->st>>>(reinterpret_cast<const W32 *>(d + b128),
                                                                 (uint32_t)S->w32.size(), table32(S));
    if (!S->side.empty()) {
        const SideOp *o = reinterpret_cast<const SideOp *>(d + b128 + b32);
        const uint32_t n = (uint32_t)S->side.size();
        k_side_claim<<<cdivu(n, ST), ST, 0, S->st>>>(o, n, S->cl, S->sst);
        k_side_write<<<cdivu(n, ST), ST, 0, S->st>>>(o, n, S->cl, S->pos);
    }
    HIP_TRY(S->w, hipGetLastError());
    S->w32.clear();
    S->w128.clear();
    S->side.clear();
    return GWAOI_OK;
}

int create(gwaoi_world *w, SyncState **out) {
    SyncState *S = new (std::nothrow) SyncState();
    if (!S) return GWAOI_ENOMEM;
    const WorldView v = world_view(w);
    S->w = w;
    S->st = v.st;
    S->max_slots = v.max_slots;
    uint32_t nbk = 512;  // buckets of three: at least 2 entries per slot
    while (3ull * nbk < 2ull * v.max_slots) nbk <<= 1;
    const uint32_t cap = 3 * nbk;
    S->hbuckets = nbk;
    S->hcap = cap;
    const size_t N = v.max_slots;
    S->oflag_cap = (uint32_t)N;
    if (int rc = alloc_all(w, S->slots, SLOT_U4 * N, S->cl, 2 * N, S->oflag, N, S->oflag_n, 1, S->htab, 4 * (size_t)nbk,
                       S->tag, N)) {
        sync_destroy(S);
        return rc;
    }
    S->sst = reinterpret_cast<uint32_t *>(S->slots.get());
    S->pos = reinterpret_cast<float4 *>(S->slots + 1);
    S->eid = S->slots + 2;
    S->cid = S->slots + 3;
    bool ok = hipMemsetAsync(S->slots, 0, N * 16 * SLOT_U4, S->st) == hipSuccess &&
              hipMemsetAsync(S->cl, 0, N * 16, S->st) == hipSuccess &&
              hipMemsetAsync(S->tag, 0, N * 4, S->st) == hipSuccess &&
              hipMemsetAsync(S->oflag_n, 0, 4, S->st) == hipSuccess &&
              hipMemsetAsync(S->htab, 0xFF, (size_t)nbk * 64, S->st) == hipSuccess &&  // every entry H_EMPTY
              S->stage_ev.create(hipEventDisableTiming) == GWAOI_OK && S->ndec_ev.create(hipEventDisableTiming) == GWAOI_OK &&
              S->h_ndec.alloc(1) == GWAOI_OK;
    if (!ok) {
        sync_destroy(S);
        return GWAOI_EDEVICE;
    }
    *S->h_ndec = 0;  // read after a wait for ndec_ev, which a failed first decode launch never records
    // space of every slot in call order (the world may hold entities already)
    std::vector<uint4> qs(N);
    for (uint32_t s = 0; s < N; ++s) qs[s] = make_uint4(NO_GATE, world_slot_space(w, s), 0u, 0u);
    if (hipMemcpy2DAsync(S->sst, 16 * SLOT_U4, qs.data(), 16, 16, N, hipMemcpyHostToDevice, S->st) != hipSuccess ||
        hipStreamSynchronize(S->st) != hipSuccess) {
        sync_destroy(S);
        return GWAOI_EDEVICE;
    }
    S->h_hkey.assign(cap, make_uint4(0, 0, 0, 0));
    S->h_hval.assign(cap, H_EMPTY);
    S->h_eid.assign(N, make_uint4(0, 0, 0, 0));
    S->h_bound.assign(N, 0);
    S->h_client.assign(N, 0);
    S->h_plain.assign(N, 0);
    S->h_bucket.assign(N, H_EMPTY);
    *out = S;
    return GWAOI_OK;
}

int state(gwaoi_world *w, SyncState **out) {
    if (!w) return GWAOI_EINVAL;
    SyncState *&S = world_sync(w);
    if (!S) {
        if (int rc = create(w, &S)) return rc;
    }
    *out = S;
    return GWAOI_OK;
}

uint4 load_id(const uint8_t *p) {
    uint4 v;
    std::memcpy(&v, p, 16);
    return v;
}

bool same(const uint4 &a, const uint4 &b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// Entry e of the id table: bucket e / 3, way e % 3 (see lookup).
uint32_t hkey_vec(uint32_t e) { return 4 * (e / 3) + e % 3; }        // uint4 index of its key
uint32_t hval_word(uint32_t e) { return 16 * (e / 3) + 12 + e % 3; }  // uint32 index of its slot
uint32_t h_first(const SyncState *S, const uint4 &id) {  // the probe's first entry
    return 3 * (id_hash(id.x, id.y, id.z, id.w) & (S->hbuckets - 1));
}
uint32_t h_next(const SyncState *S, uint32_t e) { return e + 1 == S->hcap ? 0 : e + 1; }

// entry of id, or H_EMPTY
uint32_t h_find(const SyncState *S, const uint4 &id) {
    uint32_t h = h_first(S, id);
    for (uint32_t p = 0; p < S->hcap; ++p, h = h_next(S, h)) {
        const uint32_t v = S->h_hval[h];
        if (v == H_EMPTY) return H_EMPTY;
        if (v != H_TOMB && same(S->h_hkey[h], id)) return h;
    }
    return H_EMPTY;
}

// Rebuild the table without tombstones and upload it whole.
int h_rehash(SyncState *S) {
    std::fill(S->h_hval.begin(), S->h_hval.end(), H_EMPTY);
    S->hused = 0;
    for (uint32_t s = 0; s < S->max_slots; ++s) {
        if (!S->h_bound[s]) continue;
        const uint4 id = S->h_eid[s];
        uint32_t h = h_first(S, id);
        while (S->h_hval[h] != H_EMPTY) h = h_next(S, h);
        S->h_hkey[h] = id;
        S->h_hval[h] = s;
        S->h_bucket[s] = h;
        S->hused++;
    }
    // drop pending table writes: the whole table goes up now (after the other pending writes)
    std::vector<W32> k32;
    for (const W32 &e : S->w32)
        if (e.arr != A_HVAL) k32.push_back(e);
    S->w32.swap(k32);
    std::vector<W128> k128;
    for (const W128 &e : S->w128)
        if (e.arr != B_HKEY) k128.push_back(e);
    S->w128.swap(k128);
    if (int rc = push(S)) return rc;
    S->h_tab.assign(4 * (size_t)S->hbuckets, make_uint4(H_EMPTY, H_EMPTY, H_EMPTY, H_EMPTY));
    for (uint32_t h = 0; h < S->hcap; ++h) {
        S->h_tab[hkey_vec(h)] = S->h_hkey[h];
        reinterpret_cast<uint32_t *>(S->h_tab.data())[hval_word(h)] = S->h_hval[h];
    }
    HIP_TRY(S->w, hipMemcpyAsync(S->htab, S->h_tab.data(), S->h_tab.size() * 16, hipMemcpyHostToDevice, S->st));
    HIP_TRY(S->w, hipStreamSynchronize(S->st));  // h_tab is pageable staging
    return GWAOI_OK;
}

int bind_one(SyncState *S, uint32_t slot, const uint4 &id) {
    if (slot >= S->max_slots) return GWAOI_EBADSLOT;
    const uint32_t hb = h_find(S, id);
    if (S->h_bound[slot]) return (hb != H_EMPTY && S->h_hval[hb] == slot) ? GWAOI_OK : GWAOI_ESTATE;
    if (hb != H_EMPTY) return GWAOI_ESTATE;  // id bound to another slot
    if (S->hused + 1 > S->hcap / 4 * 3) {
        // too many tombstones (live entries are <= max_slots <= hcap/2)
        if (int rc = h_rehash(S)) return rc;
    }
    uint32_t h = h_first(S, id);
    while (S->h_hval[h] != H_EMPTY && S->h_hval[h] != H_TOMB) h = h_next(S, h);
    if (S->h_hval[h] == H_EMPTY) S->hused++;
    S->h_hkey[h] = id;
    S->h_hval[h] = slot;
    S->h_bucket[slot] = h;
    S->h_bound[slot] = 1;
    S->h_eid[slot] = id;
    put128(S, B_HKEY, hkey_vec(h), id);
    put32(S, A_HVAL, hval_word(h), slot);
    put128(S, B_EID, slot, id);
    return GWAOI_OK;
}

int ensure_u32(SyncState *S, DevBuf<uint32_t> &b, size_t n) {
    if (n <= b.cap()) return GWAOI_OK;
    return alloc_all(S->w, b, std::max<size_t>(n + n / 4, 1024));
}

// (device) records, grown to n uint4
int ensure_out(SyncState *S, DevBuf<uint4> &b, size_t n) {
    if (n <= b.cap()) return GWAOI_OK;
    return alloc_all(S->w, b, std::max<size_t>(n + n / 8, 3 * 1024));
}

int ensure_host(SyncState *S, PinnedBuf<uint8_t> &b, size_t bytes) {
    if (bytes <= b.cap()) return GWAOI_OK;
    return alloc_pinned(S->w, b, std::max<size_t>(bytes + bytes / 8, 1 << 16));
}

// Multisplit bases: blk_cnt [parts][nb] -> exclusive scan (parts*nb + 1
// entries, the last is the total) -> h_off_raw[0..parts].
int fetch_bases(SyncState *S, uint32_t parts, bool sync);

unsigned long long unpack_bases(SyncState *S, uint32_t parts) {  // -> the extra word
    const unsigned long long *h = reinterpret_cast<const unsigned long long *>(S->h_offp.get());
    S->h_off_raw.assign(h, h + parts + 1);
    return h[parts + 1];
}

// per-part bases of the [parts][nb] counts in blk_cnt (scanned in place) into d_off[0, parts],
// with *extra (a device word, e.g. a cursor) in d_off[parts + 1]
int part_bases(SyncState *S, uint32_t parts, uint32_t nb, bool sync = true, bool copy = true,
               const unsigned long long *extra = nullptr) {
    const size_t n = (size_t)parts * nb + 1;
    if (int rc = ensure_u32(S, S->scan_tmp, scan_tmp_elems(n) + 4)) return rc;
    if (parts + 2 > S->d_off.cap())
        if (int rc = alloc_all(S->w, S->d_off, parts + 2)) return rc;
    scan_exclusive(S->blk_cnt, S->blk_cnt, n, S->scan_tmp, S->st);
    k_part_offsets<<<cdivu(parts + 1, ST), ST, 0, S->st>>>(S->blk_cnt, parts, nb, S->d_off, extra);
    HIP_TRY(S->w, hipGetLastError());
    return copy ? fetch_bases(S, parts, sync) : GWAOI_OK;
}

// the bases part_bases left in d_off (and the extra word), to pinned host memory; unpack_bases
// turns them into h_off_raw once the stream has reached the copy
int fetch_bases(SyncState *S, uint32_t parts, bool sync) {
    if (int rc = ensure_host(S, S->h_offp, (parts + 2) * 8)) return rc;
    HIP_TRY(S->w, hipMemcpyAsync(S->h_offp, S->d_off, (parts + 2) * 8, hipMemcpyDeviceToHost, S->st));
    if (sync) {
        HIP_TRY(S->w, hipStreamSynchronize(S->st));
        unpack_bases(S, parts);
    }
    return GWAOI_OK;
}

void fill_out(SyncState *S, gwaoi_gate_records *o, const std::vector<uint64_t> &off, const uint8_t *rec) {
    o->n_gates = (uint32_t)S->gate_ids.size();
    o->gate_ids = S->gate_ids.data();
    o->offsets = off.data();
    o->records = rec;
}

int collect_sync(gwaoi_world *w, gwaoi_gate_records *out, bool to_host) {
    if (!w || !out) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = state(w, &S)) return rc;
    const WorldView v = world_view(w);
    if (v.pending_ops) return GWAOI_ESTATE;
    if (int rc = push(S)) return rc;
    // flagged slots outside the frame get their own-client record only (InterestedBy is empty
    // outside an AOI space): the host ops' list, then the slots k_decode listed
    std::vector<uint32_t> left;
    std::sort(S->left.begin(), S->left.end());
    S->left.erase(std::unique(S->left.begin(), S->left.end()), S->left.end());
    for (uint32_t s : S->left)
        if (world_slot_space(w, s) == SP_DEAD) left.push_back(s);
    S->left.clear();
    uint32_t n_dec = 0;
    if (S->decoded) {  // copied behind the last decode: done by now unless that flush is still running
        HIP_TRY(S->w, hipEventSynchronize(S->ndec_ev));
        n_dec = *S->h_ndec;
        S->decoded = false;
        n_dec = std::min(n_dec, S->oflag_cap);  // k_decode lists a slot at most once (atomicOr claim)
    }
    const size_t n_left = left.size() + n_dec;
    if (n_left) {
        if (int rc = ensure_u32(S, S->d_left, n_left)) return rc;
        if (!left.empty())
            HIP_TRY(S->w, hipMemcpyAsync(S->d_left, left.data(), left.size() * 4, hipMemcpyHostToDevice, S->st));
        if (n_dec) {
            HIP_TRY(S->w, hipMemcpyAsync(S->d_left + left.size(), S->oflag, (size_t)n_dec * 4, hipMemcpyDeviceToDevice,
                                  S->st));
            HIP_TRY(S->w, hipMemsetAsync(S->oflag_n, 0, 4, S->st));
        }
    }
    const uint32_t G = (uint32_t)S->gate_ids.size();
    const uint32_t n_ent = v.F.n + (uint32_t)n_left;
    const uint32_t nb = std::max(1u, cdivu(n_ent, ST));
    FanArgs A{};
    A.F = v.F;
    A.info = v.info;
    A.left = S->d_left;
    A.n_left = (uint32_t)n_left;
    A.eid = S->eid;
    A.cid = S->cid;
    A.sst = S->sst;
    A.pos = S->pos;
    A.G = G;
    A.nb = nb;
    if (int rc = ensure_u32(S, S->blk_cnt, (size_t)G * nb + 1)) return rc;
    A.blk_cnt = S->blk_cnt;
    if (n_ent > S->f_snd.cap()) {
        const size_t c = std::max<size_t>(n_ent + n_ent / 8, 1024);
        if (int rc = alloc_all(S->w, S->f_snd, c, S->f_rg, c, S->f_rec, 2 * c, S->f_frec, c, S->f_cid, c, S->f_cnt, c,
                               S->f_sb, c))
            return rc;
    }
    int rc_scr = GWAOI_OK;
    if (!S->scr_cursor && (rc_scr = alloc_all(S->w, S->scr_cursor, 1))) return rc_scr;
    A.fcnt = S->f_cnt;
    A.fsb = S->f_sb;
    A.snd = S->f_snd;
    A.rg = S->f_rg;
    A.srec = S->f_rec;
    A.frec = S->f_frec;
    A.fcid = S->f_cid;
    A.scr_cursor = S->scr_cursor;
    if (n_ent) k_fan_prep<<<cdivu(n_ent, ST), ST, 0, S->st>>>(A);  // also clears the flags
    uint64_t total = 0;
    S->h_off_raw.assign((size_t)G + 1, 0);  // G gates, all empty unless the passes below run
    if (G && n_ent) {
        // pass 1: hits into the scratch; a run past the capacity is redone after a regrow
        for (int attempt = 0;; ++attempt) {
            if (!S->scr && (rc_scr = ensure_u32(S, S->scr, 32 * (size_t)n_ent))) return rc_scr;
            A.scr = S->scr;
            A.scr_cap = std::min<unsigned long long>(S->scr.cap(), SCR_FULL - 1ull);
            if (attempt) {  // (k_fan_prep zeroed them for the first)
                HIP_TRY(S->w, hipMemsetAsync(S->scr_cursor, 0, 8, S->st));
                HIP_TRY(S->w, hipMemsetAsync(S->blk_cnt + (size_t)G * nb, 0, 4, S->st));
            }
            k_fan_hits_wave<<<nb, ST, (size_t)G * 4, S->st>>>(A);
            HIP_TRY(S->w, hipGetLastError());
            // the per-gate bases are scanned before the capacity check: one host round trip
            // for both (a rerun rewrites every count the scan read).  The write pass follows on
            // the device with the output as it is (the last collect's size), queued before the
            // (pageable, host-blocking) copies of the bases and the cursor; it writes nothing
            // when either capacity fell short, which the host sees below
            if (int rc = part_bases(S, G, nb, false, false, S->scr_cursor)) return rc;
            A.out = S->out;
            A.out_recs = S->out.cap() / 3;
#ifdef GWAOI_EXP_FW_ROUNDTRIP  // A/B: the write pass launched after the host's sync (before round 6)
            A.out_recs = 0;
#endif
            if (A.out_recs) {
                k_fan_write<<<nb, ST, (3 * (size_t)G + 1) * 4, S->st>>>(A);
                HIP_TRY(S->w, hipGetLastError());
            }
            if (int rc = fetch_bases(S, G, false)) return rc;
            HIP_TRY(S->w, hipStreamSynchronize(S->st));
            const unsigned long long used = unpack_bases(S, G);
            if (used <= A.scr_cap) break;
            if (attempt || used >= SCR_FULL) {
                world_set_error(w, "sync: fan-out scratch exceeds 2^32 entries");
                return GWAOI_ENOMEM;
            }
            if ((rc_scr = ensure_u32(S, S->scr, (size_t)used))) return rc_scr;
        }
        total = S->h_off_raw[G];
    }
    if (total > A.out_recs) {  // (first collect, or more records than the output holds)
        if (int rc = ensure_out(S, S->out, 3 * total)) return rc;
        A.out = S->out;
        A.out_recs = S->out.cap() / 3;
        k_fan_write<<<nb, ST, (3 * (size_t)G + 1) * 4, S->st>>>(A);
        HIP_TRY(S->w, hipGetLastError());
    }
    if (int rc = ensure_out(S, S->out, 3)) return rc;  // (an empty collect's pointer)
    S->h_off.assign(S->h_off_raw.begin(), S->h_off_raw.end());
    if (to_host) {
        if (int rc = ensure_host(S, S->h_rec, std::max<uint64_t>(total, 1) * 48)) return rc;
        if (total) HIP_TRY(S->w, hipMemcpyAsync(S->h_rec, S->out, total * 48, hipMemcpyDeviceToHost, S->st));
        HIP_TRY(S->w, hipStreamSynchronize(S->st));
        fill_out(S, out, S->h_off, S->h_rec);
    } else {
        fill_out(S, out, S->h_off, reinterpret_cast<const uint8_t *>(S->out.get()));
    }
    return GWAOI_OK;
}

// gwaoi_collect_broadcast(_device): messages (slots[m], flags[m]) in host or device memory.
// Reads the state of the last flush and changes none of it.
int collect_cast(gwaoi_world *w, const uint32_t *slots, const uint32_t *flags, size_t n, gwaoi_gate_records *out,
                 bool on_device) {
    if (!w || !out || (n && !slots)) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = state(w, &S)) return rc;
    const WorldView v = world_view(w);
    if (v.pending_ops) return GWAOI_ESTATE;
    if (n > 0x7FFFFFFFull) return GWAOI_EINVAL;
    if (!on_device)  // nothing is produced on error: checked before any device work
        for (size_t m = 0; m < n; ++m) {
            if (flags && (flags[m] & ~(GWAOI_CAST_OWN | GWAOI_CAST_NEIGHBORS))) return GWAOI_EINVAL;
            if (slots[m] >= S->max_slots) return GWAOI_EBADSLOT;
        }
    if (int rc = push(S)) return rc;
    const uint32_t G = (uint32_t)S->gate_ids.size();
    S->h_off_cast.assign((size_t)G + 1, 0);
    uint64_t total = 0;
    int status = GWAOI_OK;
    if (G && n) {
        CastArgs A{};
        A.F = v.F;
        A.info = v.info;
        A.slots = S->slots;
        if (on_device) {
            A.m_slot = slots;
            A.m_flags = flags;
        } else {
            if (int rc = ensure_u32(S, S->cast_in, 2 * n)) return rc;
            HIP_TRY(S->w, hipMemcpyAsync(S->cast_in, slots, n * 4, hipMemcpyHostToDevice, S->st));
            if (flags) HIP_TRY(S->w, hipMemcpyAsync(S->cast_in + n, flags, n * 4, hipMemcpyHostToDevice, S->st));
            A.m_slot = S->cast_in;
            A.m_flags = flags ? S->cast_in + n : nullptr;
        }
        A.n = (uint32_t)n;
        A.max_slots = S->max_slots;
        // a block loops over a contiguous chunk of messages, its waves every (ST / 64)-th one; the
        // grid is capped so that the [G][nb] table stays bounded.  Both passes take these.
        A.per = std::max<uint32_t>(ST / 64, (cdivu(n, CAST_MAX_BLOCKS) + ST / 64 - 1) / (ST / 64) * (ST / 64));
        A.nb = cdivu(n, A.per);
        A.G = G;
        if (int rc = ensure_u32(S, S->blk_cnt, (size_t)G * A.nb + 1)) return rc;
        A.blk_cnt = S->blk_cnt;
        if (!S->cast_sc)
            if (int rc = alloc_all(S->w, S->cast_sc, 1)) return rc;
        A.sc = S->cast_sc;
        HIP_TRY(S->w, hipMemsetAsync(S->cast_sc, 0, 8, S->st));
        k_cast_count<<<A.nb, ST, (size_t)G * 4, S->st>>>(A);
        HIP_TRY(S->w, hipGetLastError());
        // as the fan-out: the bases are scanned and the write pass queued with the output as it
        // is (the last broadcast's size) before the one host wait, which brings the per-gate
        // bases, the 64-bit total and the device form's error bits
        if (int rc = part_bases(S, G, A.nb, false, false, S->cast_sc)) return rc;
        A.out = S->cast_out;
        A.out_recs = S->cast_out.cap() / 2;
        if (A.out_recs) {
            k_cast_write<<<A.nb, ST, (size_t)G * 4, S->st>>>(A);
            HIP_TRY(S->w, hipGetLastError());
        }
        if (int rc = fetch_bases(S, G, false)) return rc;
        HIP_TRY(S->w, hipStreamSynchronize(S->st));
        const unsigned long long sc = unpack_bases(S, G);
        if (sc & CAST_E_FLAGS) status = GWAOI_EINVAL;
        if (sc & CAST_E_SLOT) status = GWAOI_EBADSLOT;
        total = sc & CAST_TOTAL;
        if (total > 0xFFFFFFFFull) {
            world_set_error(w, "sync: a broadcast of more than 2^32 - 1 records");
            return GWAOI_ECAPACITY;
        }
        if (total > A.out_recs) {  // (first broadcast, or more records than the output holds)
            if (int rc = ensure_out(S, S->cast_out, 2 * total)) return rc;
            A.out = S->cast_out;
            A.out_recs = S->cast_out.cap() / 2;
            k_cast_write<<<A.nb, ST, (size_t)G * 4, S->st>>>(A);
            HIP_TRY(S->w, hipGetLastError());
        }
        S->h_off_cast.assign(S->h_off_raw.begin(), S->h_off_raw.end());
    }
    if (int rc = ensure_out(S, S->cast_out, 2)) return rc;  // (an empty result's pointer)
    if (!on_device) {
        if (int rc = ensure_host(S, S->h_cast, std::max<uint64_t>(total, 1) * GWAOI_CAST_REC)) return rc;
        if (total)
            HIP_TRY(S->w, hipMemcpyAsync(S->h_cast, S->cast_out, total * GWAOI_CAST_REC, hipMemcpyDeviceToHost, S->st));
        HIP_TRY(S->w, hipStreamSynchronize(S->st));
        fill_out(S, out, S->h_off_cast, S->h_cast);
    } else {
        HIP_TRY(S->w, hipStreamSynchronize(S->st));  // (the caller's arrays are free to go; the records are complete)
        fill_out(S, out, S->h_off_cast, reinterpret_cast<const uint8_t *>(S->cast_out.get()));
    }
    if (status != GWAOI_OK) world_set_error(w, "sync: broadcast messages with a bad slot or flag were dropped");
    return status;
}

// gwaoi_collect_client_switch: messages (slots[m], gate_ids[m], clientids[16m..16m+16)) in host
// memory.  Reads the relation of the last flush and the clients on the device; the clients are
// switched behind the write pass.  Every error is found before anything changes.
int collect_switch(gwaoi_world *w, const uint32_t *slots, const uint16_t *gate_ids, const uint8_t *clientids, size_t n,
                   gwaoi_gate_records *creates, gwaoi_gate_records *destroys) {
    if (!w || !creates || !destroys || (n && (!slots || !gate_ids))) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = state(w, &S)) return rc;
    const WorldView v = world_view(w);
    if (v.pending_ops) return GWAOI_ESTATE;
    if (n > 0x7FFFFFFFull) return GWAOI_EINVAL;
    for (size_t m = 0; m < n; ++m)
        if (slots[m] >= S->max_slots) return GWAOI_EBADSLOT;
    if (S->sw_stamp.empty()) S->sw_stamp.assign(S->max_slots, 0u);
    if (++S->sw_epoch == 0) {  // (the stamps of 2^32 calls ago)
        std::fill(S->sw_stamp.begin(), S->sw_stamp.end(), 0u);
        S->sw_epoch = 1;
    }
    for (size_t m = 0; m < n; ++m) {
        if (S->sw_stamp[slots[m]] == S->sw_epoch) return GWAOI_EINVAL;  // a slot named twice: the caller splits the batch
        S->sw_stamp[slots[m]] = S->sw_epoch;
    }
    // the new clients' gate indices; gates the world has not seen are registered only once the
    // whole batch is known to fit
    const uint32_t G0 = (uint32_t)S->gate_ids.size();
    std::vector<uint16_t> fresh;
    std::unordered_map<uint32_t, uint32_t> fresh_idx;
    static const uint8_t zero_id[GWAOI_ID_LEN] = {0};
    S->sw_gate.assign(n, NO_GATE);
    for (size_t m = 0; m < n; ++m) {
        if (!clientids || !std::memcmp(clientids + GWAOI_ID_LEN * m, zero_id, GWAOI_ID_LEN)) continue;  // no client
        auto it = S->gate_idx.find(gate_ids[m]);
        if (it != S->gate_idx.end()) {
            S->sw_gate[m] = it->second;
            continue;
        }
        auto ins = fresh_idx.emplace(gate_ids[m], G0 + (uint32_t)fresh.size());
        if (ins.second) fresh.push_back(gate_ids[m]);
        S->sw_gate[m] = ins.first->second;
    }
    if (G0 + fresh.size() > GWAOI_MAX_GATES) return GWAOI_ECAPACITY;
    if (int rc = push(S)) return rc;  // every earlier gwaoi_entity_set_client is visible to the passes
    for (uint16_t id : fresh) {
        S->gate_idx.emplace(id, (uint32_t)S->gate_ids.size());
        S->gate_ids.push_back(id);
    }
    const uint32_t G = (uint32_t)S->gate_ids.size();
    uint64_t nc = 0, nd = 0;
    SwitchArgs A{};
    auto records = [&]() -> int {  // the two outputs on the device and their offsets; changes no state
        S->h_off_swc.assign((size_t)G + 1, 0);
        S->h_off_swd.assign((size_t)G + 1, 0);
        if (G && n) {
            // the messages, uploaded once: new ClientIDs, slots, new gate indices
            const size_t bytes = n * (sizeof(uint4) + 8);
            if (int rc = ensure_stage(S, bytes)) return rc;
            char *h = S->h_stage, *d = S->d_stage;
            if (clientids)
                std::memcpy(h, clientids, n * 16);
            else
                std::memset(h, 0, n * 16);
            std::memcpy(h + n * 16, slots, n * 4);
            std::memcpy(h + n * 20, S->sw_gate.data(), n * 4);
            HIP_TRY(S->w, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, S->st));
            HIP_TRY(S->w, hipEventRecord(S->stage_ev, S->st));
            S->stage_pending = true;
            A.F = v.F;
            A.info = v.info;
            A.slots = S->slots;
            A.m_cid = reinterpret_cast<const uint4 *>(d);
            A.m_slot = reinterpret_cast<const uint32_t *>(d + n * 16);
            A.m_gate = reinterpret_cast<const uint32_t *>(d + n * 20);
            A.n = (uint32_t)n;
            // the broadcast's grid: a block loops over a contiguous chunk of messages, capped so that
            // the [2][G][nb] table stays bounded
            A.per = std::max<uint32_t>(ST / 64, (cdivu(n, CAST_MAX_BLOCKS) + ST / 64 - 1) / (ST / 64) * (ST / 64));
            A.nb = cdivu(n, A.per);
            A.G = G;
            if (int rc = ensure_u32(S, S->blk_cnt, 2 * (size_t)G * A.nb + 1)) return rc;
            A.blk_cnt = S->blk_cnt;
            if (!S->sw_sc)
                if (int rc = alloc_all(S->w, S->sw_sc, 2)) return rc;
            if (!S->h_sw_sc)
                if (int rc = alloc_pinned(S->w, S->h_sw_sc, 2)) return rc;
            A.sc = S->sw_sc;
            const size_t lds = 2 * (size_t)G * 4;
            HIP_TRY(S->w, hipMemsetAsync(S->sw_sc, 0, 16, S->st));
            k_switch_count<<<A.nb, ST, lds, S->st>>>(A);
            HIP_TRY(S->w, hipGetLastError());
            // as the broadcast: the bases are scanned and the write pass queued with the outputs as
            // they are (the last switch's sizes) before the one host wait, which brings the per-gate
            // bases and the two 64-bit totals
            if (int rc = part_bases(S, 2 * G, A.nb, false, false)) return rc;
            auto write = [&]() -> int {
                A.out_c = S->sw_out_c;
                A.out_d = S->sw_out_d;
                A.cap_c = S->sw_out_c.cap() / 3;
                A.cap_d = S->sw_out_d.cap() / 2;
                k_switch_write<<<A.nb, ST, lds, S->st>>>(A);
                HIP_TRY(S->w, hipGetLastError());
                return GWAOI_OK;
            };
            const bool queued = S->sw_out_c.cap() && S->sw_out_d.cap();
            if (queued)
                if (int rc = write()) return rc;
            if (int rc = fetch_bases(S, 2 * G, false)) return rc;
            HIP_TRY(S->w, hipMemcpyAsync(S->h_sw_sc, S->sw_sc, 16, hipMemcpyDeviceToHost, S->st));
            HIP_TRY(S->w, hipStreamSynchronize(S->st));
            unpack_bases(S, 2 * G);
            nc = S->h_sw_sc[0];
            nd = S->h_sw_sc[1];
            if (nc + nd > 0xFFFFFFFFull) {  // (either kind alone, or the two in their one index space)
                world_set_error(w, "sync: a client switch of more than 2^32 - 1 records");
                return GWAOI_ECAPACITY;
            }
            if (!queued || nc > A.cap_c || nd > A.cap_d) {  // (first switch, or more records than an output holds)
                if (int rc = ensure_out(S, S->sw_out_c, 3 * std::max<uint64_t>(nc, 1))) return rc;
                if (int rc = ensure_out(S, S->sw_out_d, 2 * std::max<uint64_t>(nd, 1))) return rc;
                if (nc + nd)
                    if (int rc = write()) return rc;
            }
            const uint64_t split = S->h_off_raw[G];  // creates occupy [0, split) of one index space
            for (uint32_t g = 0; g <= G; ++g) {
                S->h_off_swc[g] = S->h_off_raw[g];
                S->h_off_swd[g] = S->h_off_raw[G + g] - split;
            }
        }
        if (int rc = ensure_out(S, S->sw_out_c, 3)) return rc;  // (an empty result's pointers)
        if (int rc = ensure_out(S, S->sw_out_d, 2)) return rc;
        if (int rc = ensure_host(S, S->h_sw_c, std::max<uint64_t>(nc, 1) * GWAOI_SYNC_OUT_REC)) return rc;
        return ensure_host(S, S->h_sw_d, std::max<uint64_t>(nd, 1) * GWAOI_DESTROY_REC);
    };
    if (int rc = records()) {  // nothing is changed: the batch's gates go again
        for (uint16_t id : fresh) S->gate_idx.erase(id);
        S->gate_ids.resize(G0);
        return rc;
    }
    if (nc) HIP_TRY(S->w, hipMemcpyAsync(S->h_sw_c, S->sw_out_c, nc * GWAOI_SYNC_OUT_REC, hipMemcpyDeviceToHost, S->st));
    if (nd) HIP_TRY(S->w, hipMemcpyAsync(S->h_sw_d, S->sw_out_d, nd * GWAOI_DESTROY_REC, hipMemcpyDeviceToHost, S->st));
    // the switch itself, behind the write pass on the same stream: what n gwaoi_entity_set_client
    // calls would have left.  (Without a gate no slot ever had a client and the batch attaches
    // none: nothing to write.)
    if (G && n) {
        k_switch_apply<<<cdivu(n, ST), ST, 0, S->st>>>(A.m_cid, A.m_slot, A.m_gate, A.n, S->slots);
        HIP_TRY(S->w, hipGetLastError());
    }
    for (size_t m = 0; m < n; ++m) S->h_client[slots[m]] = S->sw_gate[m] != NO_GATE;
    HIP_TRY(S->w, hipStreamSynchronize(S->st));
    fill_out(S, creates, S->h_off_swc, S->h_sw_c);
    fill_out(S, destroys, S->h_off_swd, S->h_sw_d);
    return GWAOI_OK;
}

// `need` bytes (256-B aligned) of the current flush's arena: device memory that stays alive until
// the flush that consumes the batch built in it (older chunks were consumed by earlier flushes).
int arena_take(SyncState *S, size_t need, char **base) {
    uint64_t ticks_now;
    {
        gwaoi_info inf;
        gwaoi_world_info(S->w, &inf);
        ticks_now = inf.ticks;
    }
    if (S->arena_tick != ticks_now) {
        if (S->arena.size() > 1) {  // keep the largest chunk only
            HIP_TRY(S->w, hipStreamSynchronize(S->st));
            std::sort(S->arena.begin(), S->arena.end(),
                      [](const SyncState::Chunk &a, const SyncState::Chunk &b) { return a.buf.cap() > b.buf.cap(); });
            S->arena.erase(S->arena.begin() + 1, S->arena.end());
        }
        for (auto &c : S->arena) c.used = 0;
        S->arena_tick = ticks_now;
    }
    SyncState::Chunk *ch = nullptr;
    for (auto &c : S->arena)
        if (c.buf.cap() - c.used >= need) {
            ch = &c;
            break;
        }
    if (!ch) {
        SyncState::Chunk c{};
        if (alloc_all(S->w, c.buf, std::max<size_t>(need, 1 << 20))) return GWAOI_EDEVICE;
        S->arena.push_back(std::move(c));
        ch = &S->arena.back();
    }
    *base = ch->buf + ch->used;
    ch->used += need;
    return GWAOI_OK;
}

int decode(gwaoi_world *w, const uint8_t *payload, size_t n, bool on_device) {
    if (!w || (n && !payload)) return GWAOI_EINVAL;
    if (on_device && (reinterpret_cast<uintptr_t>(payload) & 15u)) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = state(w, &S)) return rc;
    if (world_view(w).in_flight) return GWAOI_ESTATE;  // a flush in flight reads the sync state's stream
    if (!n) return GWAOI_OK;
    if (n > 0x7FFFFFFFull) return GWAOI_EINVAL;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t need = 6 * al(n * 4) + al(4) + (on_device ? 0 : al(n * 32));
    char *base;
    if (int rc = arena_take(S, need, &base)) return rc;
    uint32_t *o_slot = reinterpret_cast<uint32_t *>(base);
    float *o_x = reinterpret_cast<float *>(base + al(n * 4));
    float *o_z = reinterpret_cast<float *>(base + 2 * al(n * 4));
    uint32_t *o_sp = reinterpret_cast<uint32_t *>(base + 3 * al(n * 4));
    uint32_t *o_ys = reinterpret_cast<uint32_t *>(base + 4 * al(n * 4));
    const uint4 *pay;
    if (on_device) {
        pay = reinterpret_cast<const uint4 *>(payload);
    } else {
        char *dp = base + 6 * al(n * 4) + al(4);
        HIP_TRY(S->w, hipMemcpyAsync(dp, payload, n * 32, hipMemcpyHostToDevice, S->st));
        pay = reinterpret_cast<const uint4 *>(dp);
    }
    if (int rc = push(S)) return rc;
    DecodeArgs A{};
    A.pay = pay;
    A.n = (uint32_t)n;
    A.htab = S->htab;
    A.hmask = S->hbuckets - 1;
    A.sst = S->sst;
    A.o_slot = o_slot;
    A.o_sp = o_sp;
    A.o_x = o_x;
    A.o_z = o_z;
    A.o_ys = o_ys;
    A.claim0 = S->claim_next;
    A.cl = S->cl;
    A.pos = S->pos;
    A.oflag = S->oflag;
    A.oflag_n = S->oflag_n;
    A.h_ndec = S->h_ndec;
    A.oflag_cap = S->oflag_cap;
    A.dups = reinterpret_cast<uint32_t *>(base + 5 * al(n * 4));
    A.ndup = reinterpret_cast<uint32_t *>(base + 6 * al(n * 4));
    S->claim_next += n;
    S->decoded = true;
    k_decode<GWAOI_DEC_PER><<<cdivu(n, ST * GWAOI_DEC_PER), ST, 0, S->st>>>(A);
    k_decode_apply<<<cdivu(n, ST), ST, 0, S->st>>>(A);
    k_decode_dups<<<std::min<uint32_t>(cdivu(n, ST), 64u), ST, 0, S->st>>>(A);
    HIP_TRY(S->w, hipGetLastError());
    HIP_TRY(S->w, hipEventRecord(S->ndec_ev, S->st));
    return world_queue_decoded(w, o_slot, o_x, o_z, o_sp, n);
}

// gwaoi_steer_batch(_device): the decode's shape.  The batch arrays, the host form's uploaded
// messages and its answers on the device all come from the flush's arena.
int steer(gwaoi_world *w, const uint32_t *movers, const uint32_t *targets, const float *steps, const uint32_t *flags,
          size_t n, uint8_t *out_applied, float *out_pos, bool on_device) {
    if (!w || (n && (!movers || !targets || !steps || !out_applied || !out_pos))) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = state(w, &S)) return rc;
    const WorldView v = world_view(w);
    if (v.pending_ops) return GWAOI_ESTATE;  // (a flush in flight counts: the relation and the frame of one flush)
    if (n > 0x7FFFFFFFull) return GWAOI_EINVAL;
    if (!on_device) {  // nothing happens on error: checked before any device work
        int bad = GWAOI_OK;
        for (size_t m = 0; m < n && bad != GWAOI_EBADSLOT; ++m) {
            if (movers[m] >= v.max_slots || (targets[m] >= v.max_slots && targets[m] != GWAOI_NO_SLOT))
                bad = GWAOI_EBADSLOT;
            else if (flags && (flags[m] & ~STEER_ALL))
                bad = GWAOI_EINVAL;
            else if (!std::isfinite(steps[m]) && bad == GWAOI_OK)
                bad = GWAOI_ENONFINITE;
        }
        if (bad == GWAOI_EBADSLOT || bad == GWAOI_EINVAL) return bad;
        if (S->sw_stamp.empty()) S->sw_stamp.assign(S->max_slots, 0u);
        if (++S->sw_epoch == 0) {  // (the stamps of 2^32 calls ago)
            std::fill(S->sw_stamp.begin(), S->sw_stamp.end(), 0u);
            S->sw_epoch = 1;
        }
        for (size_t m = 0; m < n; ++m) {
            if (S->sw_stamp[movers[m]] == S->sw_epoch) return GWAOI_EINVAL;  // a mover named twice
            S->sw_stamp[movers[m]] = S->sw_epoch;
        }
        if (bad != GWAOI_OK) return bad;  // GWAOI_ENONFINITE, the last in precedence
    }
    if (!n) return GWAOI_OK;
    if (!S->h_steer)
        if (int rc = alloc_pinned(S->w, S->h_steer, 1)) return rc;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t a4 = al(n * 4);
    const size_t need = 5 * a4 + al(4) + (on_device ? 0 : 4 * a4 + al(n) + al(n * 16));
    char *base;
    if (int rc = arena_take(S, need, &base)) return rc;
    if (int rc = push(S)) return rc;  // every earlier position and yaw write is visible
    SteerArgs A{};
    A.F = v.F;
    A.info = v.info;
    A.slots = S->slots;
    A.n = (uint32_t)n;
    A.max_slots = v.max_slots;
    A.o_slot = reinterpret_cast<uint32_t *>(base);
    A.o_x = reinterpret_cast<float *>(base + a4);
    A.o_z = reinterpret_cast<float *>(base + 2 * a4);
    A.o_sp = reinterpret_cast<uint32_t *>(base + 3 * a4);
    A.o_ms = reinterpret_cast<uint32_t *>(base + 4 * a4);
    A.status = reinterpret_cast<uint32_t *>(base + 5 * a4);
    if (on_device) {
        A.mv = movers;
        A.tg = targets;
        A.step = steps;
        A.flags = flags;
        A.out_applied = out_applied;
        A.out_pos = out_pos;
    } else {
        char *in = base + 5 * a4 + al(4);
        HIP_TRY(S->w, hipMemcpyAsync(in, movers, n * 4, hipMemcpyHostToDevice, S->st));
        HIP_TRY(S->w, hipMemcpyAsync(in + a4, targets, n * 4, hipMemcpyHostToDevice, S->st));
        HIP_TRY(S->w, hipMemcpyAsync(in + 2 * a4, steps, n * 4, hipMemcpyHostToDevice, S->st));
        if (flags) HIP_TRY(S->w, hipMemcpyAsync(in + 3 * a4, flags, n * 4, hipMemcpyHostToDevice, S->st));
        A.mv = reinterpret_cast<const uint32_t *>(in);
        A.tg = reinterpret_cast<const uint32_t *>(in + a4);
        A.step = reinterpret_cast<const float *>(in + 2 * a4);
        A.flags = flags ? reinterpret_cast<const uint32_t *>(in + 3 * a4) : nullptr;
        A.out_applied = reinterpret_cast<uint8_t *>(in + 4 * a4);
        A.out_pos = reinterpret_cast<float *>(in + 4 * a4 + al(n));
    }
    A.claim0 = S->claim_next;
    A.cl = S->cl;
    A.sst = S->sst;
    A.pos = S->pos;
    S->claim_next += n;
    HIP_TRY(S->w, hipMemsetAsync(A.status, 0, 4, S->st));
    k_steer<<<cdivu(n, ST), ST, 0, S->st>>>(A);
    k_steer_apply<<<cdivu(n, ST), ST, 0, S->st>>>(A);
    HIP_TRY(S->w, hipGetLastError());
    if (!on_device) {
        HIP_TRY(S->w, hipMemcpyAsync(out_applied, A.out_applied, n, hipMemcpyDeviceToHost, S->st));
        HIP_TRY(S->w, hipMemcpyAsync(out_pos, A.out_pos, n * 16, hipMemcpyDeviceToHost, S->st));
    }
    // the one host wait: the status word (and, in the host form, the answers)
    HIP_TRY(S->w, hipMemcpyAsync(S->h_steer, A.status, 4, hipMemcpyDeviceToHost, S->st));
    HIP_TRY(S->w, hipStreamSynchronize(S->st));
    const uint32_t status = *S->h_steer;
    if (int rc = world_queue_decoded(w, A.o_slot, A.o_x, A.o_z, A.o_sp, n)) return rc;
    if (status & STEER_E_SLOT) {
        world_set_error(w, "steer: messages with a slot >= max_slots are dropped");
        return GWAOI_EBADSLOT;
    }
    if (status & STEER_E_INVAL) {
        world_set_error(w, "steer: a flag bit outside MOVE | FACE, or a mover named twice (one of its messages applied)");
        return GWAOI_EINVAL;
    }
    if (status & STEER_E_NONFINITE) {
        world_set_error(w, "steer: messages with a non-finite step or a non-finite new position are dropped");
        return GWAOI_ENONFINITE;
    }
    return GWAOI_OK;
}

}  // namespace

// Buffers of the interest-set reads.  The world's own (world_query), apart from SyncState: the
// rows and membership reads need no sync layer and must not create one.
struct QueryState {
    DevBuf<uint32_t> in;             // the host forms' uploaded queries
    DevBuf<uint32_t> cnt, scan_tmp;  // rows: n + 1 lengths, scanned in place into the offsets
    DevBuf<uint32_t> items;          // rows: neighbour slots (valid until the next rows call)
    DevBuf<unsigned long long> sc;   // 64-bit total | Q_E_SLOT
    PinnedBuf<unsigned long long> h_sc;
    PinnedBuf<uint32_t> h_off, h_items;  // the host form's rows
    DevBuf<uint32_t> out;            // the host forms' membership / nearest answers on the device
    // range reads: results of their own (valid until the next range call, whatever the rows calls do)
    DevBuf<uint32_t> r_cnt, r_items;
    DevBuf<float> r_dists;
    PinnedBuf<uint32_t> h_roff, h_ritems, h_rdists;  // (h_rdists holds floats)
};

void query_destroy(QueryState *Q) { delete Q; }  // (the world has synchronised its streams)

namespace {

int query_state(gwaoi_world *w, QueryState **out) {
    QueryState *&Q = world_query(w);
    if (!Q) {
        Q = new (std::nothrow) QueryState();
        if (!Q) return GWAOI_ENOMEM;
    }
    if (!Q->sc)
        if (int rc = alloc_all(w, Q->sc, 1)) return rc;
    if (!Q->h_sc)
        if (int rc = alloc_pinned(w, Q->h_sc, 1)) return rc;
    *out = Q;
    return GWAOI_OK;
}

template <class T>
int q_ensure(gwaoi_world *w, DevBuf<T> &b, size_t n) {
    if (n <= b.cap()) return GWAOI_OK;
    return alloc_all(w, b, std::max<size_t>(n + n / 4, 1024));
}
int q_ensure_host(gwaoi_world *w, PinnedBuf<uint32_t> &b, size_t n) {
    if (n <= b.cap()) return GWAOI_OK;
    return alloc_pinned(w, b, std::max<size_t>(n + n / 8, 1 << 14));
}

// one wave per query: a block loops over a contiguous chunk, its waves every (ST / 64)-th one,
// and the grid is capped as the broadcast's
uint32_t query_chunk(size_t n) {
    return std::max<uint32_t>(ST / 64, (cdivu(n, CAST_MAX_BLOCKS) + ST / 64 - 1) / (ST / 64) * (ST / 64));
}

// the total | error word to the host: the call's host wait
int query_sc(gwaoi_world *w, QueryState *Q, hipStream_t st, unsigned long long *sc) {
    HIP_TRY(w, hipMemcpyAsync(Q->h_sc, Q->sc, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(w, hipStreamSynchronize(st));
    *sc = *Q->h_sc;
    return GWAOI_OK;
}

// gwaoi_neighbors_batch(_device): reads only the frame.
int query_rows(gwaoi_world *w, const uint32_t *slots, size_t n, gwaoi_slot_rows *out, bool on_device) {
    if (!w || !out || (n && !slots)) return GWAOI_EINVAL;
    const WorldView v = world_view(w);
    if (v.pending_ops) return GWAOI_ESTATE;
    if (n > 0x7FFFFFFFull) return GWAOI_EINVAL;
    if (!on_device)  // nothing is produced on error: checked before any device work
        for (size_t m = 0; m < n; ++m)
            if (slots[m] >= v.max_slots) return GWAOI_EBADSLOT;
    QueryState *Q;
    if (int rc = query_state(w, &Q)) return rc;
    if (int rc = q_ensure(w, Q->cnt, n + 1)) return rc;
    if (int rc = q_ensure(w, Q->items, 1)) return rc;  // (an empty result's pointer)
    uint64_t total = 0;
    int status = GWAOI_OK;
    if (n) {
        RowsArgs A{};
        A.F = v.F;
        A.info = v.info;
        if (on_device) {
            A.q_slot = slots;
        } else {
            if (int rc = q_ensure(w, Q->in, n)) return rc;
            HIP_TRY(w, hipMemcpyAsync(Q->in, slots, n * 4, hipMemcpyHostToDevice, v.st));
            A.q_slot = Q->in;
        }
        A.n = (uint32_t)n;
        A.max_slots = v.max_slots;
        A.per = query_chunk(n);
        const uint32_t nb = cdivu(n, A.per);
        A.cnt = Q->cnt;
        A.sc = Q->sc;
        if (int rc = q_ensure(w, Q->scan_tmp, scan_tmp_elems(n + 1) + 4)) return rc;
        HIP_TRY(w, hipMemsetAsync(Q->sc, 0, 8, v.st));
        k_rows_count<<<nb, ST, 0, v.st>>>(A);
        HIP_TRY(w, hipGetLastError());
        scan_exclusive(Q->cnt, Q->cnt, n + 1, Q->scan_tmp, v.st);
        // the write pass is queued with the items as they are (the last call's size) before the one
        // host wait, which brings the 64-bit total and the device form's error bit
        A.items = Q->items;
        A.cap = Q->items.cap();
        k_rows_write<<<nb, ST, 0, v.st>>>(A);
        HIP_TRY(w, hipGetLastError());
        unsigned long long sc;
        if (int rc = query_sc(w, Q, v.st, &sc)) return rc;
        if (sc & Q_E_SLOT) status = GWAOI_EBADSLOT;
        total = sc & Q_TOTAL;
        if (total > 0xFFFFFFFFull) {
            world_set_error(w, "query: rows of more than 2^32 - 1 items");
            return GWAOI_ECAPACITY;
        }
        if (total > A.cap) {  // (the write pass declined: more items than the output holds)
            if (int rc = q_ensure(w, Q->items, total)) return rc;
            A.items = Q->items;
            A.cap = Q->items.cap();
            k_rows_write<<<nb, ST, 0, v.st>>>(A);
            HIP_TRY(w, hipGetLastError());
            if (on_device) HIP_TRY(w, hipStreamSynchronize(v.st));  // (the rows are complete on return)
        }
    } else {
        HIP_TRY(w, hipMemsetAsync(Q->cnt, 0, 4, v.st));
        if (on_device) HIP_TRY(w, hipStreamSynchronize(v.st));
    }
    out->n = (uint32_t)n;
    if (on_device) {
        out->offsets = Q->cnt;
        out->items = Q->items;
    } else {
        if (int rc = q_ensure_host(w, Q->h_off, n + 1)) return rc;
        if (int rc = q_ensure_host(w, Q->h_items, std::max<uint64_t>(total, 1))) return rc;
        HIP_TRY(w, hipMemcpyAsync(Q->h_off, Q->cnt, (n + 1) * 4, hipMemcpyDeviceToHost, v.st));
        if (total) HIP_TRY(w, hipMemcpyAsync(Q->h_items, Q->items, total * 4, hipMemcpyDeviceToHost, v.st));
        HIP_TRY(w, hipStreamSynchronize(v.st));
        out->offsets = Q->h_off;
        out->items = Q->h_items;
    }
    if (status != GWAOI_OK) world_set_error(w, "query: rows of a slot >= max_slots are empty");
    return status;
}

// gwaoi_related_batch(_device): reads only the frame.
int query_related(gwaoi_world *w, const uint32_t *a, const uint32_t *b, size_t n, uint8_t *out, bool on_device) {
    if (!w || (n && (!a || !b || !out))) return GWAOI_EINVAL;
    const WorldView v = world_view(w);
    if (v.pending_ops) return GWAOI_ESTATE;
    if (n > 0x7FFFFFFFull) return GWAOI_EINVAL;
    if (!on_device)
        for (size_t m = 0; m < n; ++m)
            if (a[m] >= v.max_slots || b[m] >= v.max_slots) return GWAOI_EBADSLOT;
    if (!n) return GWAOI_OK;
    QueryState *Q;
    if (int rc = query_state(w, &Q)) return rc;
    RelatedArgs A{};
    A.F = v.F;
    A.info = v.info;
    if (on_device) {
        A.qa = a;
        A.qb = b;
        A.out = out;
    } else {
        if (int rc = q_ensure(w, Q->in, 2 * n)) return rc;
        if (int rc = q_ensure(w, Q->out, n / 4 + 1)) return rc;
        HIP_TRY(w, hipMemcpyAsync(Q->in, a, n * 4, hipMemcpyHostToDevice, v.st));
        HIP_TRY(w, hipMemcpyAsync(Q->in + n, b, n * 4, hipMemcpyHostToDevice, v.st));
        A.qa = Q->in;
        A.qb = Q->in + n;
        A.out = reinterpret_cast<uint8_t *>(Q->out.get());
    }
    A.n = (uint32_t)n;
    A.max_slots = v.max_slots;
    A.sc = Q->sc;
    HIP_TRY(w, hipMemsetAsync(Q->sc, 0, 8, v.st));
    k_related<<<cdivu(n, ST), ST, 0, v.st>>>(A);
    HIP_TRY(w, hipGetLastError());
    if (!on_device) HIP_TRY(w, hipMemcpyAsync(out, A.out, n, hipMemcpyDeviceToHost, v.st));
    unsigned long long sc;
    if (int rc = query_sc(w, Q, v.st, &sc)) return rc;
    if (sc & Q_E_SLOT) {
        world_set_error(w, "query: pairs with a slot >= max_slots are not related");
        return GWAOI_EBADSLOT;
    }
    return GWAOI_OK;
}

// gwaoi_nearest_batch(_device): the frame, the tags and the slots' y (the sync layer's).
int query_nearest(gwaoi_world *w, const uint32_t *slots, const uint32_t *masks, const uint32_t *wants, size_t n,
                  uint32_t *out_slot, float *out_dist, bool on_device) {
    if (!w || (n && (!slots || !out_slot || !out_dist || (masks && !wants)))) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = state(w, &S)) return rc;
    const WorldView v = world_view(w);
    if (v.pending_ops) return GWAOI_ESTATE;
    if (n > 0x7FFFFFFFull) return GWAOI_EINVAL;
    if (!on_device)
        for (size_t m = 0; m < n; ++m)
            if (slots[m] >= v.max_slots) return GWAOI_EBADSLOT;
    if (!n) return GWAOI_OK;
    QueryState *Q;
    if (int rc = query_state(w, &Q)) return rc;
    if (int rc = push(S)) return rc;  // every earlier tag and position write is visible
    NearArgs A{};
    A.F = v.F;
    A.info = v.info;
    A.slots = S->slots;
    A.tag = S->tag;
    if (on_device) {
        A.q_slot = slots;
        A.q_mask = masks;
        A.q_want = masks ? wants : nullptr;
        A.out_slot = out_slot;
        A.out_dist = out_dist;
    } else {
        if (int rc = q_ensure(w, Q->in, 3 * n)) return rc;
        if (int rc = q_ensure(w, Q->out, 2 * n)) return rc;
        HIP_TRY(w, hipMemcpyAsync(Q->in, slots, n * 4, hipMemcpyHostToDevice, v.st));
        if (masks) {
            HIP_TRY(w, hipMemcpyAsync(Q->in + n, masks, n * 4, hipMemcpyHostToDevice, v.st));
            HIP_TRY(w, hipMemcpyAsync(Q->in + 2 * n, wants, n * 4, hipMemcpyHostToDevice, v.st));
        }
        A.q_slot = Q->in;
        A.q_mask = masks ? Q->in + n : nullptr;
        A.q_want = masks ? Q->in + 2 * n : nullptr;
        A.out_slot = Q->out;
        A.out_dist = reinterpret_cast<float *>(Q->out + n);
    }
    A.n = (uint32_t)n;
    A.max_slots = v.max_slots;
    A.per = query_chunk(n);
    A.sc = Q->sc;
    HIP_TRY(w, hipMemsetAsync(Q->sc, 0, 8, v.st));
    k_nearest<<<cdivu(n, A.per), ST, 0, v.st>>>(A);
    HIP_TRY(w, hipGetLastError());
    if (!on_device) {
        HIP_TRY(w, hipMemcpyAsync(out_slot, A.out_slot, n * 4, hipMemcpyDeviceToHost, v.st));
        HIP_TRY(w, hipMemcpyAsync(out_dist, A.out_dist, n * 4, hipMemcpyDeviceToHost, v.st));
    }
    unsigned long long sc;
    if (int rc = query_sc(w, Q, v.st, &sc)) return rc;
    if (sc & Q_E_SLOT) {
        world_set_error(w, "query: sources with a slot >= max_slots have no nearest neighbour");
        return GWAOI_EBADSLOT;
    }
    return GWAOI_OK;
}

int range_status(gwaoi_world *w, unsigned long long sc) {
    if (!(sc & ~RANGE_TOTAL)) return GWAOI_OK;
    world_set_error(w, "range: rows of queries with a bad slot, space, flag, radius or point are empty");
    return (sc & Q_E_SLOT) ? GWAOI_EBADSLOT : (sc & Q_E_SPACE) ? GWAOI_EBADSPACE : (sc & Q_E_INVAL) ? GWAOI_EINVAL : GWAOI_ENONFINITE;
}

// gwaoi_range_batch / gwaoi_range_count_batch (_device): the frame, the tags and the slots' y (the
// sync layer's).  out == nullptr is the count form: the count pass alone, its n answers in counts.
int query_range(gwaoi_world *w, const gwaoi_range_query *q, size_t n, gwaoi_range_rows *out, uint32_t *counts,
                bool count_only, bool on_device) {
    if (!w || (count_only ? (n && !counts) : !out) || (n && !q)) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = state(w, &S)) return rc;
    const WorldView v = world_view(w);
    if (v.pending_ops) return GWAOI_ESTATE;
    if (n > 0x7FFFFFFFull) return GWAOI_EINVAL;
    if (on_device) {
        if (n && (reinterpret_cast<uintptr_t>(q) & 15u)) return GWAOI_EINVAL;  // (two 16-B loads per query)
    } else {  // nothing is produced on error: checked before any device work
        for (size_t m = 0; m < n; ++m) {
            const gwaoi_range_query &x = q[m];
            if (x.flags & ~(GWAOI_RANGE_POINT | GWAOI_RANGE_PLANAR)) return GWAOI_EINVAL;
            if (!std::isfinite(x.radius)) return GWAOI_ENONFINITE;
            if (x.radius < 0.0f) return GWAOI_EINVAL;  // (-0.0 is 0)
            if (x.flags & GWAOI_RANGE_POINT) {
                if (!std::isfinite(x.x) || !std::isfinite(x.y) || !std::isfinite(x.z)) return GWAOI_ENONFINITE;
                if (!world_space_used(w, x.center)) return GWAOI_EBADSPACE;
            } else if (x.center >= v.max_slots) {
                return GWAOI_EBADSLOT;
            }
        }
    }
    if (n && (unsigned long long)n * v.F.n > RANGE_TOTAL) {  // (the total shares its word with the error bits)
        world_set_error(w, "range: more queries times entities than the total can count");
        return GWAOI_ECAPACITY;
    }
    QueryState *Q;
    if (int rc = query_state(w, &Q)) return rc;
    RangeArgs A{};
    if (n) {
        if (int rc = push(S)) return rc;  // every earlier tag and position write is visible
        A.F = v.F;
        A.info = v.info;
        A.slots = S->slots;
        A.tag = S->tag;
        if (on_device) {
            A.q = reinterpret_cast<const uint4 *>(q);
        } else {
            if (int rc = q_ensure(w, Q->in, 8 * n)) return rc;
            HIP_TRY(w, hipMemcpyAsync(Q->in, q, n * sizeof(gwaoi_range_query), hipMemcpyHostToDevice, v.st));
            A.q = reinterpret_cast<const uint4 *>(Q->in.get());
        }
        A.n = (uint32_t)n;
        A.max_slots = v.max_slots;
        A.max_spaces = v.max_spaces;
        A.n_grids = v.n_grids;
        A.per = query_chunk(n);
        A.sc = Q->sc;
    }
    const uint32_t nb = n ? cdivu(n, A.per) : 0u;
    if (count_only) {  // one launch, one host wait, one copy
        if (!n) return GWAOI_OK;
        if (!on_device)
            if (int rc = q_ensure(w, Q->out, n)) return rc;
        A.cnt = on_device ? counts : Q->out.get();
        A.scan = 0u;
        HIP_TRY(w, hipMemsetAsync(Q->sc, 0, 8, v.st));
        k_range_count<<<nb, ST, 0, v.st>>>(A);
        HIP_TRY(w, hipGetLastError());
        if (!on_device) HIP_TRY(w, hipMemcpyAsync(counts, A.cnt, n * 4, hipMemcpyDeviceToHost, v.st));
        unsigned long long sc;
        if (int rc = query_sc(w, Q, v.st, &sc)) return rc;
        return range_status(w, sc);
    }
    if (int rc = q_ensure(w, Q->r_cnt, n + 1)) return rc;
    if (int rc = q_ensure(w, Q->r_items, 1)) return rc;  // (an empty result's pointers)
    if (int rc = q_ensure(w, Q->r_dists, 1)) return rc;
    uint64_t total = 0;
    int status = GWAOI_OK;
    if (n) {
        A.cnt = Q->r_cnt;
        A.scan = 1u;
        if (int rc = q_ensure(w, Q->scan_tmp, scan_tmp_elems(n + 1) + 4)) return rc;
        HIP_TRY(w, hipMemsetAsync(Q->sc, 0, 8, v.st));
        k_range_count<<<nb, ST, 0, v.st>>>(A);
        HIP_TRY(w, hipGetLastError());
        scan_exclusive(Q->r_cnt, Q->r_cnt, n + 1, Q->scan_tmp, v.st);
        // the write pass is queued with the outputs as they are (the last call's size) before the one
        // host wait, which brings the total and the device form's error bits
        A.items = Q->r_items;
        A.dists = Q->r_dists;
        A.cap = std::min(Q->r_items.cap(), Q->r_dists.cap());
        k_range_write<<<nb, ST, 0, v.st>>>(A);
        HIP_TRY(w, hipGetLastError());
        unsigned long long sc;
        if (int rc = query_sc(w, Q, v.st, &sc)) return rc;
        status = range_status(w, sc);
        total = sc & RANGE_TOTAL;
        if (total > 0xFFFFFFFFull) {
            world_set_error(w, "range: rows of more than 2^32 - 1 items");
            return GWAOI_ECAPACITY;
        }
        if (total > A.cap) {  // (the write pass declined: items and dists regrow together)
            if (int rc = q_ensure(w, Q->r_items, total)) return rc;
            if (int rc = q_ensure(w, Q->r_dists, total)) return rc;
            A.items = Q->r_items;
            A.dists = Q->r_dists;
            A.cap = std::min(Q->r_items.cap(), Q->r_dists.cap());
            k_range_write<<<nb, ST, 0, v.st>>>(A);
            HIP_TRY(w, hipGetLastError());
            if (on_device) HIP_TRY(w, hipStreamSynchronize(v.st));  // (the rows are complete on return)
        }
    } else {
        HIP_TRY(w, hipMemsetAsync(Q->r_cnt, 0, 4, v.st));
        if (on_device) HIP_TRY(w, hipStreamSynchronize(v.st));
    }
    out->n = (uint32_t)n;
    if (on_device) {
        out->offsets = Q->r_cnt;
        out->items = Q->r_items;
        out->dists = Q->r_dists;
    } else {
        if (int rc = q_ensure_host(w, Q->h_roff, n + 1)) return rc;
        if (int rc = q_ensure_host(w, Q->h_ritems, std::max<uint64_t>(total, 1))) return rc;
        if (int rc = q_ensure_host(w, Q->h_rdists, std::max<uint64_t>(total, 1))) return rc;
        HIP_TRY(w, hipMemcpyAsync(Q->h_roff, Q->r_cnt, (n + 1) * 4, hipMemcpyDeviceToHost, v.st));
        if (total) {
            HIP_TRY(w, hipMemcpyAsync(Q->h_ritems, Q->r_items, total * 4, hipMemcpyDeviceToHost, v.st));
            HIP_TRY(w, hipMemcpyAsync(Q->h_rdists, Q->r_dists, total * 4, hipMemcpyDeviceToHost, v.st));
        }
        HIP_TRY(w, hipStreamSynchronize(v.st));
        out->offsets = Q->h_roff;
        out->items = Q->h_ritems;
        out->dists = reinterpret_cast<const float *>(Q->h_rdists.get());
    }
    return status;
}

int set_tags(gwaoi_world *w, const uint32_t *slots, const uint32_t *tags, size_t n) {
    if (!w || (n && (!slots || !tags))) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = state(w, &S)) return rc;
    for (size_t i = 0; i < n; ++i)
        if (slots[i] >= S->max_slots) return GWAOI_EBADSLOT;
    for (size_t i = 0; i < n; ++i) put32(S, A_TAG, slots[i], tags[i]);  // (push keeps a slot's last write)
    return GWAOI_OK;
}

}  // namespace

void sync_note_slot(SyncState *S, uint32_t slot, uint32_t space_or_dead) {
    put32(S, A_QSPACE, slot, space_or_dead);
    if (space_or_dead == SP_DEAD)
        S->left.push_back(slot);
    else  // Space.enter: syncInfoFlag |= sifSyncOwnClient | sifSyncNeighborClients (Space.go:205)
        S->side.push_back(SideOp{slot, SIDE_SIF, 0ull, make_float4(0.f, 0.f, 0.f, 0.f)});
}

bool sync_slot_plain(const SyncState *S, uint32_t slot) { return slot < S->max_slots && S->h_plain[slot]; }

void sync_destroy(SyncState *S) {
    if (!S) return;
    if (S->st) (void)hipStreamSynchronize(S->st);
    delete S;
}

}  // namespace gw

// =============================================================== C ABI =======

using gw::SyncState;

extern "C" {

int gwaoi_entity_bind(gwaoi_world *w, uint32_t slot, const uint8_t eid[GWAOI_ID_LEN]) {
    return gw::api_guard([&]() -> int {
    if (!w || !eid) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = gw::state(w, &S)) return rc;
    return gw::bind_one(S, slot, gw::load_id(eid));
    });
}

int gwaoi_entity_bind_batch(gwaoi_world *w, const uint32_t *slots, const uint8_t *eids, size_t n) {
    return gw::api_guard([&]() -> int {
    if (!w || (n && (!slots || !eids))) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = gw::state(w, &S)) return rc;
    for (size_t i = 0; i < n; ++i)
        if (int rc = gw::bind_one(S, slots[i], gw::load_id(eids + 16 * i))) return rc;
    return GWAOI_OK;
    });
}

int gwaoi_entity_unbind(gwaoi_world *w, uint32_t slot) {
    return gw::api_guard([&]() -> int {
    if (!w) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = gw::state(w, &S)) return rc;
    if (slot >= S->max_slots) return GWAOI_EBADSLOT;
    if (!S->h_bound[slot]) return GWAOI_ESTATE;
    const uint32_t h = S->h_bucket[slot];
    S->h_hval[h] = gw::H_TOMB;
    gw::put32(S, gw::A_HVAL, gw::hval_word(h), gw::H_TOMB);
    S->h_bound[slot] = 0;
    S->h_bucket[slot] = gw::H_EMPTY;
    if (S->h_client[slot]) {
        S->h_client[slot] = 0;
        gw::put32(S, gw::A_CGATE, slot, gw::NO_GATE);
    }
    gw::put32(S, gw::A_SYNCING, slot, 0);
    gw::put32(S, gw::A_TAG, slot, 0);
    return GWAOI_OK;
    });
}

int gwaoi_entity_set_client(gwaoi_world *w, uint32_t slot, uint16_t gate_id, const uint8_t *clientid) {
    return gw::api_guard([&]() -> int {
    if (!w) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = gw::state(w, &S)) return rc;
    if (slot >= S->max_slots) return GWAOI_EBADSLOT;
    if (!clientid) {
        S->h_client[slot] = 0;
        gw::put32(S, gw::A_CGATE, slot, gw::NO_GATE);
        return GWAOI_OK;
    }
    auto it = S->gate_idx.find(gate_id);
    uint32_t g;
    if (it == S->gate_idx.end()) {
        if (S->gate_ids.size() >= GWAOI_MAX_GATES) return GWAOI_ECAPACITY;
        g = (uint32_t)S->gate_ids.size();
        S->gate_idx.emplace(gate_id, g);
        S->gate_ids.push_back(gate_id);
    } else {
        g = it->second;
    }
    S->h_client[slot] = 1;
    gw::put128(S, gw::B_CID, slot, gw::load_id(clientid));
    gw::put32(S, gw::A_CGATE, slot, g);
    return GWAOI_OK;
    });
}

int gwaoi_entity_set_syncing(gwaoi_world *w, uint32_t slot, int syncing) {
    return gw::api_guard([&]() -> int {
    if (!w) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = gw::state(w, &S)) return rc;
    if (slot >= S->max_slots) return GWAOI_EBADSLOT;
    gw::put32(S, gw::A_SYNCING, slot, syncing ? 1u : 0u);
    return GWAOI_OK;
    });
}

int gwaoi_entity_set_position_yaw(gwaoi_world *w, uint32_t slot, float x, float y, float z, float yaw) {
    return gw::api_guard([&]() -> int {
    if (!w) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = gw::state(w, &S)) return rc;
    if (slot >= S->max_slots) return GWAOI_EBADSLOT;
    S->side.push_back(gw::SideOp{slot, gw::SIDE_POS | gw::SIDE_YAW, S->claim_next++, make_float4(x, y, z, yaw)});
    return GWAOI_OK;
    });
}

int gwaoi_set_position_yaw(gwaoi_world *w, uint32_t slot, float x, float y, float z, float yaw) {
    return gw::api_guard([&]() -> int {
    if (!w) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = gw::state(w, &S)) return rc;
    if (slot >= S->max_slots) return GWAOI_EBADSLOT;
    if (gw::world_slot_space(w, slot) != gw::SP_DEAD) {  // Space.move of an AOI space: Position + Moved
        if (int rc = gwaoi_moved(w, slot, x, z)) return rc;
        S->side.push_back(gw::SideOp{slot, gw::SIDE_POS | gw::SIDE_YAW | gw::SIDE_SIF, S->claim_next++,
                                     make_float4(x, y, z, yaw)});
        return GWAOI_OK;
    }
    // nilSpace or a space without AOI: Space.move returns before Position (Space.go:253-257); yaw
    // and both flags are still set (Entity.go:1196-1204)
    S->side.push_back(gw::SideOp{slot, gw::SIDE_YAW | gw::SIDE_SIF, S->claim_next++, make_float4(x, y, z, yaw)});
    S->left.push_back(slot);
    return GWAOI_OK;
    });
}

int gwaoi_entity_enter_plain(gwaoi_world *w, uint32_t slot, float x, float y, float z) {
    return gw::api_guard([&]() -> int {
    if (!w) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = gw::state(w, &S)) return rc;
    if (slot >= S->max_slots) return GWAOI_EBADSLOT;
    // Space.enter panics unless the entity is in nilSpace (Space.go:193-195)
    if (S->h_plain[slot] || gw::world_slot_space(w, slot) != gw::SP_DEAD) return GWAOI_ESTATE;
    S->h_plain[slot] = 1;
    S->side.push_back(gw::SideOp{slot, gw::SIDE_POS | gw::SIDE_SIF, S->claim_next++, make_float4(x, y, z, 0.f)});
    S->left.push_back(slot);
    return GWAOI_OK;
    });
}

int gwaoi_entity_leave_plain(gwaoi_world *w, uint32_t slot) {
    return gw::api_guard([&]() -> int {
    if (!w) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = gw::state(w, &S)) return rc;
    if (slot >= S->max_slots) return GWAOI_EBADSLOT;
    if (!S->h_plain[slot]) return GWAOI_ESTATE;  // Space.leave panics for another space (Space.go:229-231)
    S->h_plain[slot] = 0;
    return GWAOI_OK;
    });
}

int gwaoi_sync_from_clients(gwaoi_world *w, const uint8_t *payload, size_t n_rec) {
    return gw::api_guard([&]() -> int {
    return gw::decode(w, payload, n_rec, false);
    });
}

int gwaoi_sync_from_clients_device(gwaoi_world *w, const uint8_t *d_payload, size_t n_rec) {
    return gw::api_guard([&]() -> int {
    return gw::decode(w, d_payload, n_rec, true);
    });
}

int gwaoi_collect_sync_infos(gwaoi_world *w, gwaoi_gate_records *out) { return gw::api_guard([&]() -> int { return gw::collect_sync(w, out, true); }); }

int gwaoi_collect_sync_infos_device(gwaoi_world *w, gwaoi_gate_records *out) {
    return gw::api_guard([&]() -> int {
    return gw::collect_sync(w, out, false);
    });
}

int gwaoi_collect_broadcast(gwaoi_world *w, const uint32_t *slots, const uint32_t *flags, size_t n,
                            gwaoi_gate_records *out) {
    return gw::api_guard([&]() -> int {
    return gw::collect_cast(w, slots, flags, n, out, false);
    });
}

int gwaoi_collect_broadcast_device(gwaoi_world *w, const uint32_t *d_slots, const uint32_t *d_flags, size_t n,
                                   gwaoi_gate_records *out) {
    return gw::api_guard([&]() -> int {
    return gw::collect_cast(w, d_slots, d_flags, n, out, true);
    });
}

int gwaoi_collect_client_switch(gwaoi_world *w, const uint32_t *slots, const uint16_t *gate_ids,
                                const uint8_t *clientids, size_t n, gwaoi_gate_records *creates,
                                gwaoi_gate_records *destroys) {
    return gw::api_guard([&]() -> int {
    return gw::collect_switch(w, slots, gate_ids, clientids, n, creates, destroys);
    });
}

int gwaoi_neighbors_batch(gwaoi_world *w, const uint32_t *slots, size_t n, gwaoi_slot_rows *out) {
    return gw::api_guard([&]() -> int { return gw::query_rows(w, slots, n, out, false); });
}

int gwaoi_neighbors_batch_device(gwaoi_world *w, const uint32_t *d_slots, size_t n, gwaoi_slot_rows *out) {
    return gw::api_guard([&]() -> int { return gw::query_rows(w, d_slots, n, out, true); });
}

int gwaoi_related_batch(gwaoi_world *w, const uint32_t *a, const uint32_t *b, size_t n, uint8_t *out) {
    return gw::api_guard([&]() -> int { return gw::query_related(w, a, b, n, out, false); });
}

int gwaoi_related_batch_device(gwaoi_world *w, const uint32_t *d_a, const uint32_t *d_b, size_t n, uint8_t *d_out) {
    return gw::api_guard([&]() -> int { return gw::query_related(w, d_a, d_b, n, d_out, true); });
}

int gwaoi_entity_set_tag(gwaoi_world *w, uint32_t slot, uint32_t tag) {
    return gw::api_guard([&]() -> int { return gw::set_tags(w, &slot, &tag, 1); });
}

int gwaoi_entity_set_tag_batch(gwaoi_world *w, const uint32_t *slots, const uint32_t *tags, size_t n) {
    return gw::api_guard([&]() -> int { return gw::set_tags(w, slots, tags, n); });
}

int gwaoi_nearest_batch(gwaoi_world *w, const uint32_t *slots, const uint32_t *masks, const uint32_t *wants,
                        size_t n, uint32_t *out_slot, float *out_dist) {
    return gw::api_guard([&]() -> int { return gw::query_nearest(w, slots, masks, wants, n, out_slot, out_dist, false); });
}

int gwaoi_nearest_batch_device(gwaoi_world *w, const uint32_t *d_slots, const uint32_t *d_masks,
                               const uint32_t *d_wants, size_t n, uint32_t *d_out_slot, float *d_out_dist) {
    return gw::api_guard([&]() -> int {
    return gw::query_nearest(w, d_slots, d_masks, d_wants, n, d_out_slot, d_out_dist, true);
    });
}

int gwaoi_range_batch(gwaoi_world *w, const gwaoi_range_query *q, size_t n, gwaoi_range_rows *out) {
    return gw::api_guard([&]() -> int { return gw::query_range(w, q, n, out, nullptr, false, false); });
}

int gwaoi_range_batch_device(gwaoi_world *w, const gwaoi_range_query *d_q, size_t n, gwaoi_range_rows *out) {
    return gw::api_guard([&]() -> int { return gw::query_range(w, d_q, n, out, nullptr, false, true); });
}

int gwaoi_range_count_batch(gwaoi_world *w, const gwaoi_range_query *q, size_t n, uint32_t *out_counts) {
    return gw::api_guard([&]() -> int { return gw::query_range(w, q, n, nullptr, out_counts, true, false); });
}

int gwaoi_range_count_batch_device(gwaoi_world *w, const gwaoi_range_query *d_q, size_t n, uint32_t *d_out_counts) {
    return gw::api_guard([&]() -> int { return gw::query_range(w, d_q, n, nullptr, d_out_counts, true, true); });
}

int gwaoi_steer_batch(gwaoi_world *w, const uint32_t *movers, const uint32_t *targets, const float *steps,
                      const uint32_t *flags, size_t n, uint8_t *out_applied, float *out_pos) {
    return gw::api_guard([&]() -> int { return gw::steer(w, movers, targets, steps, flags, n, out_applied, out_pos, false); });
}

int gwaoi_steer_batch_device(gwaoi_world *w, const uint32_t *d_movers, const uint32_t *d_targets, const float *d_steps,
                             const uint32_t *d_flags, size_t n, uint8_t *d_out_applied, float *d_out_pos) {
    return gw::api_guard([&]() -> int {
    return gw::steer(w, d_movers, d_targets, d_steps, d_flags, n, d_out_applied, d_out_pos, true);
    });
}

int gwaoi_collect_client_events(gwaoi_world *w, gwaoi_gate_records *creates, gwaoi_gate_records *destroys) {
    return gw::api_guard([&]() -> int {
    using namespace gw;
    if (!w || !creates || !destroys) return GWAOI_EINVAL;
    SyncState *S;
    if (int rc = state(w, &S)) return rc;
    const WorldView v = world_view(w);
    if (v.pending_ops) return GWAOI_ESTATE;
    if (int rc = push(S)) return rc;
    const uint32_t G = (uint32_t)S->gate_ids.size();
    const uint64_t n_total = v.n_enter + v.n_leave;
    S->h_off_c.assign(G + 1, 0);
    S->h_off_d.assign(G + 1, 0);
    uint64_t nc = 0, nd = 0;
    if (G && n_total) {
        const uint32_t nb = cdivu(n_total, ST);
        if (int rc = ensure_u32(S, S->blk_cnt, 2 * (size_t)G * nb + 1)) return rc;
        RouteArgs A{};
        A.ev = v.events;
        A.n_enter = (uint32_t)v.n_enter;
        A.n_total = (uint32_t)n_total;
        A.F = v.F;
        A.info = v.info;
        A.eid = S->eid;
        A.cid = S->cid;
        A.sst = S->sst;
        A.pos = S->pos;
        A.G = G;
        A.nb = nb;
        A.blk_cnt = S->blk_cnt;
        const size_t lds = 2 * (size_t)G * 4;
        HIP_TRY(S->w, hipMemsetAsync(S->blk_cnt + 2 * (size_t)G * nb, 0, 4, S->st));
        k_route<0><<<nb, ST, lds, S->st>>>(A);
        HIP_TRY(S->w, hipGetLastError());
        if (int rc = part_bases(S, 2 * G, nb)) return rc;
        const uint64_t split = S->h_off_raw[G];  // creates occupy [0, split) of one index space
        nc = split;
        nd = S->h_off_raw[2 * G] - split;
        if (int rc = ensure_out(S, S->out, 3 * std::max<uint64_t>(nc, 1))) return rc;
        if (int rc = ensure_out(S, S->out_d, 2 * std::max<uint64_t>(nd, 1))) return rc;
        A.out_c = S->out;
        A.out_d = S->out_d;
        A.split = (uint32_t)split;
        k_route<1><<<nb, ST, lds, S->st>>>(A);
        HIP_TRY(S->w, hipGetLastError());
        for (uint32_t g = 0; g <= G; ++g) {
            S->h_off_c[g] = S->h_off_raw[g];
            S->h_off_d[g] = S->h_off_raw[G + g] - split;
        }
    }
    if (int rc = ensure_host(S, S->h_rec, std::max<uint64_t>(nc, 1) * 48)) return rc;
    if (int rc = ensure_host(S, S->h_rec_d, std::max<uint64_t>(nd, 1) * 32)) return rc;
    if (nc) HIP_TRY(S->w, hipMemcpyAsync(S->h_rec, S->out, nc * 48, hipMemcpyDeviceToHost, S->st));
    if (nd) HIP_TRY(S->w, hipMemcpyAsync(S->h_rec_d, S->out_d, nd * 32, hipMemcpyDeviceToHost, S->st));
    HIP_TRY(S->w, hipStreamSynchronize(S->st));
    fill_out(S, creates, S->h_off_c, S->h_rec);
    fill_out(S, destroys, S->h_off_d, S->h_rec_d);
    return GWAOI_OK;
    });
}

}  // extern "C"
