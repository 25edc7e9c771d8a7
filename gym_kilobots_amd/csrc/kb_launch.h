// kb_launch.h -- the launch shape of a handle (workgroup size, contact capacity, LDS staging entries, LDS image and offsets,
// register tier, instantiation), worked out from the configuration in one function: plan_launch; and the constants and
// the two LDS images it is laid out from.  Plain C++17 without HIP (tests/test_launch_cpu.py compiles it with the system
// compiler); HIP-Clang compiles the constexpr functions for the device as well.
#pragma once
#include "kb_variant.h"

#ifndef KB_MAX_WAVES
#define KB_MAX_WAVES 8
#endif
#ifndef KB_BPT
#define KB_BPT 2
#endif
#ifndef KB_MIN_WAVES_PER_SIMD
#define KB_MIN_WAVES_PER_SIMD 4
#endif
#ifndef KB_COMPACT_WAVES_PER_SIMD
#define KB_COMPACT_WAVES_PER_SIMD 6     // the compact fixed-size kernel: 80 VGPRs, three 8-wave workgroups per CU
#endif

namespace kb {

constexpr int OBJ_LIST = 64;                           // kilobots that may touch one fixture at a time
constexpr int OT_WORDS_C = 7 + 4 * KB_MAX_POLY_VERTS;   // floats per fixture in the fixture table (kb_objects.h)
constexpr int BT_WORDS_C = 6;                          // floats per object in the body table
constexpr int MC_FIELDS_C = 37;                        // words per manifold-constraint record (kb_objects.h)

// contact classes in canonical order; +1 on E/N/NE/NW for odd base-cell parity
constexpr int CLS_SAME = 0, CLS_E = 1, CLS_N = 3, CLS_NE = 5, CLS_NW = 7, CLS_WALL = 9,
              CLS_BOT_OBJ = 10, NUM_CLS = 11;
constexpr int RK = 4;                 // rank buckets per class; the last one holds every rank >= RK-1
constexpr int MAX_WAVES = KB_MAX_WAVES;   // waves per workgroup
constexpr int BK_PER_WAVE = NUM_CLS * RK;
constexpr int BPT = KB_BPT;                // bots per thread (max): N <= BPT * blockDim.x
constexpr int CAP_LDS = 1024;         // contacts staged in LDS; denser envs stage in the global scratch slice

// number of (object, partner) candidates of M objects: pairs in lexicographic order, then (object, wall)
constexpr int mc_candidates(int M) { return M * (M - 1) / 2 + 4 * M; }

// ---- LDS layout ----------------------------------------------------------------------------------
// The small arrays come first: a few of fixed size, the bucket tables of the contact sort (they scale with the waves of
// the workgroup) and -- only in kernels with objects -- the object tables; `fixed(obj, nw)` is where the arrays that
// scale with the scene start.  Those are grouped by stride, so that every offset is (base + k * stride) of four scene
// sizes.  The kernel recomputes offsets where they are used instead of keeping ~35 of them alive in scalar registers
// for the whole launch; in the fixed-size instantiations all of this folds to constants.
namespace lds {
constexpr int A16(int x) { return (x + 15) & ~15; }
constexpr int A4(int x) { return (x + 3) & ~3; }
constexpr int MISC = 0;
constexpr int WSUM = MISC + A16(4 * 64);
constexpr int BKSTART = WSUM + A16(4 * 16);
// buckets of a workgroup of nw waves (the tables double as scratch of the island placement: >= 64 entries)
constexpr int nbk(int nw) { return nw * BK_PER_WAVE < 64 ? 64 : nw * BK_PER_WAVE; }
constexpr int bkfill(int nw) { return BKSTART + A16(4 * (nbk(nw) + 1)); }
constexpr int bkmaxrank(int nw) { return bkfill(nw) + A16(4 * nbk(nw)); }
constexpr int bklist(int nw) { return bkmaxrank(nw) + A16(4 * MAX_WAVES * NUM_CLS); }
constexpr int nlist(int nw) { return bklist(nw) + A16(2 * nbk(nw)); }
constexpr int objtab(int nw) { return nlist(nw) + 16; }   // object table: mass, shape
// object areas, relative to objtab(nw)
constexpr int OBJBODY = A16(4 * OT_WORDS_C * KB_MAX_OBJECTS);            // body table
constexpr int OBJCNT = OBJBODY + A16(4 * BT_WORDS_C * KB_MAX_OBJECTS);
constexpr int OBJLIST = OBJCNT + A16(4 * KB_MAX_OBJECTS);
constexpr int OBJW = OBJLIST + A16(2 * KB_MAX_OBJECTS * OBJ_LIST);       // angular velocity, angle, angle at the start of the substep
constexpr int OBJA = OBJW + A16(4 * KB_MAX_OBJECTS);
constexpr int OBJA0 = OBJA + A16(4 * KB_MAX_OBJECTS);
constexpr int MCMASK = OBJA0 + A16(4 * KB_MAX_OBJECTS);                  // per wave: which manifold constraints it owns (u64)
constexpr int OBJSLP = MCMASK + A16(8 * (MAX_WAVES + 1));                // sleeping: b2Body::m_sleepTime of the objects (< 0: asleep)
constexpr int OBJ_AREA = OBJSLP + A16(4 * KB_MAX_OBJECTS);
constexpr int fixed(bool obj, int nw) { return objtab(nw) + (obj ? OBJ_AREA : 0); }
// per-body 32-bit arrays (stride 4 * NB): px py vx vy x0 y0 dirCnt parent
constexpr int BODY32_COUNT = 8;
// per-contact 32-bit arrays (stride 4 * capL): sPair sInfo sAcc oldAcc;  16-bit (stride 2 * capL): cbk order oldKey
constexpr int CON32_COUNT = 4, CON16_COUNT = 3;
// per-bot 16-bit arrays (stride 2 * NP): wsOff newOff next cellOf;  8-bit (stride NP): wsCnt wsCntNew
constexpr int BOT16_COUNT = 4, BOT8_COUNT = 2;
// (fx = fixed(obj, nw))
constexpr int body32(int fx, int NB, int k) { return fx + 4 * NB * k; }
constexpr int con32(int fx, int NB, int capL, int k) { return body32(fx, NB, BODY32_COUNT) + 4 * capL * k; }
constexpr int con16(int fx, int NB, int capL, int k) { return con32(fx, NB, capL, CON32_COUNT) + 2 * capL * k; }
// (whole words: the fused sensing pass counts into newOff with 32-bit atomics, two u16 counters per word, and an odd capL --
//  3 N + 64 staging entries of an odd swarm -- leaves the three 16-bit contact arrays in front an odd number of half words long)
constexpr int bot16(int fx, int NB, int capL, int NP, int k) { return A4(con16(fx, NB, capL, CON16_COUNT)) + 2 * NP * k; }
constexpr int bot8(int fx, int NB, int capL, int NP, int k) { return bot16(fx, NB, capL, NP, BOT16_COUNT) + NP * k; }
constexpr int active(int fx, int NB, int capL, int NP) { return bot8(fx, NB, capL, NP, BOT8_COUNT); }
constexpr int islwave(int fx, int NB, int capL, int NP) { return active(fx, NB, capL, NP) + 2 * NB; }   // u8 per body: wave that sweeps its island
constexpr int head(int fx, int NB, int capL, int NP) { return (islwave(fx, NB, capL, NP) + NB + 15) & ~15; }
constexpr int mcarea(int fx, int NB, int capL, int NP, int ncell) { return (head(fx, NB, capL, NP) + 2 * ncell + 4 + 15) & ~15; }
// manifold-constraint records (objects only): MC_FIELDS words x nmc candidates, field-major
constexpr int total(int fx, int NB, int capL, int NP, int ncell, int nmc) { return (mcarea(fx, NB, capL, NP, ncell) + 4 * MC_FIELDS_C * nmc + 15) & ~15; }
}  // namespace lds

// ---- sorted-bin LDS image (round 3): every kernel without objects ------------------------------------------------------
// The broadphase is a counting sort of the kilobots by grid cell ("bins"; a hash of the cells for sparse swarms), and the
// bodies LIVE in that order for the length of a substep: pos / vel / parent / ... are indexed by the kilobot's SLOT in the
// sorted order, so the candidates of a stencil row are one contiguous run of slots (no list heads, no next pointers, no
// indirection through an id).  A contact is stored at its position in the packed warm-start list of the substep
// (newOff[owner] + slot of the owner's list), so StoreImpulses is a copy, and the previous substep's list is kept as an
// LDS image (6 B per entry) that aliases arrays which only live between the island phase and the end of the substep.
//   always            : misc | pos | vel
//   parent            : union-find (emit .. sleep bookkeeping); start-of-substep angle of the TOI candidates behind it
//   dircnt            : per-direction contact counts (find .. emit) -> island census / body depth -> startY (integrate .. TOI)
//   botA              : [wsOff | wsCnt | idOf | (cellOfSlot: hashed bins)]; startX over its front (integrate .. TOI)
//   botB              : [newOff | wsCntNew]
//   con32 x 3         : lPair lInfo lAcc   (the arrival-order scratch of the sort lies over lInfo, the neighbour counters of
//                                           the sensing pass over lAcc: both dead before the emit pass writes the records)
//   act0              : position-solver island flags of even iterations (also "island has an awake body": cleared in the
//                       drive phase, hence outside the aliased zone)
//   zone              : [act1 | islWave | lOrder | lCbk]  aliased by the warm-start image [oldAcc | oldKey]
//   binE              : bin boundaries (u16, entry i = kilobots in bins < i) -> bucket tables of the contact sort -> unused
namespace ldsb {
constexpr int A16(int x) { return (x + 15) & ~15; }
constexpr int A4(int x) { return (x + 3) & ~3; }
constexpr int pos() { return 320; }                       // (MISC 256 + WSUM 64 in front)
constexpr int vel(int NB) { return pos() + 8 * NB; }
constexpr int parent(int NB) { return vel(NB) + 8 * NB; }
constexpr int dircnt(int NB) { return parent(NB) + 4 * NB; }
constexpr int botA(int NB) { return dircnt(NB) + 4 * NB; }
constexpr int botA_size(int NB, int NP, bool hc) { return A16((5 + (hc ? 2 : 0)) * NP > 4 * NB ? (5 + (hc ? 2 : 0)) * NP : 4 * NB); }
constexpr int wsoff(int NB) { return botA(NB); }
constexpr int wscnt(int NB, int NP) { return botA(NB) + 2 * NP; }
constexpr int idof(int NB, int NP) { return botA(NB) + 3 * NP; }
constexpr int cellofslot(int NB, int NP) { return botA(NB) + 5 * NP; }
constexpr int botB(int NB, int NP, bool hc) { return botA(NB) + botA_size(NB, NP, hc); }
constexpr int newoff(int NB, int NP, bool hc) { return botB(NB, NP, hc); }
constexpr int wscntnew(int NB, int NP, bool hc) { return botB(NB, NP, hc) + 2 * NP; }
constexpr int con32(int NB, int NP, bool hc, int capL, int k) { return A16(botB(NB, NP, hc) + 3 * NP) + 4 * capL * k; }
constexpr int act0(int NB, int NP, bool hc, int capL) { return con32(NB, NP, hc, capL, 3); }
constexpr int zone(int NB, int NP, bool hc, int capL) { return act0(NB, NP, hc, capL) + NB; }      // act1 follows act0 directly
constexpr int islwave(int NB, int NP, bool hc, int capL) { return zone(NB, NP, hc, capL) + NB; }
constexpr int order(int NB, int NP, bool hc, int capL) { return A4(islwave(NB, NP, hc, capL) + NB); }
constexpr int cbk(int NB, int NP, bool hc, int capL) { return order(NB, NP, hc, capL) + A4(2 * capL); }
constexpr int oldacc(int NB, int NP, bool hc, int capL) { return A4(zone(NB, NP, hc, capL)); }
constexpr int oldkey(int NB, int NP, bool hc, int capL) { return oldacc(NB, NP, hc, capL) + 4 * capL; }
constexpr int zone_end(int NB, int NP, bool hc, int capL) {
    return cbk(NB, NP, hc, capL) + A4(2 * capL) > oldkey(NB, NP, hc, capL) + 2 * capL ? cbk(NB, NP, hc, capL) + A4(2 * capL) : oldkey(NB, NP, hc, capL) + 2 * capL;
}
constexpr int binE(int NB, int NP, bool hc, int capL) { return A16(zone_end(NB, NP, hc, capL)); }
constexpr int bin_entries(int nbin) { return (nbin + 1 + 7) & ~7; }                 // u16 entries, whole 16-byte chunks
constexpr int tables(int nw) { return lds::nlist(nw) + 16 - lds::BKSTART; }       // bucket tables, relative to binE
constexpr int binE_size(int nbin, int nw) { return A16(2 * bin_entries(nbin) > tables(nw) ? 2 * bin_entries(nbin) : tables(nw)); }
constexpr int total(int NB, int NP, bool hc, int capL, int nbin, int nw) { return binE(NB, NP, hc, capL) + binE_size(nbin, nw); }
constexpr int CAPL = 688;                                                     // staged contacts of the fixed-size kernel
}  // namespace ldsb

// ---- launch shape ------------------------------------------------------------------------------------------------------
constexpr int LDS_CU = 160 * 1024;    // LDS of a CU, and the most one workgroup may allocate
constexpr int LDS_GRANULE = 1280;     // LDS is handed out in granules: an image of 54 544 B got two workgroups per CU, one of 53 168 B three

// workgroups of `threads` threads and `lds` bytes that one CU holds at a register budget of `wps` waves per SIMD
constexpr int resident_envs(int lds, int threads, int wps) {
    const int byLds = LDS_CU / (((lds + LDS_GRANULE - 1) / LDS_GRANULE) * LDS_GRANULE);
    const int byWaves = (4 * wps) / (threads / 64);
    const int n = byLds < byWaves ? byLds : byWaves;
    return n < 1 ? (byLds >= 1 ? 1 : 0) : n;
}
// register budget of a kernel without objects: 80 VGPRs (tier 2) where that holds more envs than 128 VGPRs (tier 0)
constexpr int compact_tier(int lds, int threads) {
    return resident_envs(lds, threads, KB_COMPACT_WAVES_PER_SIMD) > resident_envs(lds, threads, KB_MIN_WAVES_PER_SIMD) ? 2 : 0;
}
// ... and the envs per CU of the better of the two budgets
constexpr int resident_envs_best(int lds, int threads) { return resident_envs(lds, threads, compact_tier(lds, threads) ? KB_COMPACT_WAVES_PER_SIMD : KB_MIN_WAVES_PER_SIMD); }

// what of a configuration decides its launch shape
struct PlanInput {
    int num_bots, num_objects, num_fixtures;
    bool all_discs;                     // objects, and every fixture a circle
    int drive_mode, light_type;
    bool sense, allow_sleep;            // sense_radius > 0; allow_sleep
    int ncell, contact_capacity;        // cells of the arena's broadphase grid; kb_config.contact_capacity (0: derived)
    int threads;                        // workgroup size asked for by kb_set_block_threads; 0: kb_create chooses
};
// KB_OK, else KB_EINVAL / KB_ELDS and why; the shape goes into Params (cap ... botlaw_off) and kb_sim (threads, variant);
// tier: register budget of the kernels without objects (kb_variant.h: Shape)
struct Plan {
    int status; const char *msg;
    int cap, capL, nhead, hmask, threads, lds_total, islmin_off, botlaw_off, tier;
    Variant variant;
};

// the sorted-bin image: its bytes, and where the per-island minimum of the sleep times (NB words, SLEEP kernels, idle
// arrays between the position sweeps and the continuous step) lies -- over the bin boundaries, else over the staged pairs,
// else behind the image
struct BinsImage { int bytes, islmin_off; };
constexpr BinsImage bins_image(int NB, int NP, bool hashed, int capL, int nhead, int nw, bool sleep) {
    BinsImage b{ldsb::total(NB, NP, hashed, capL, nhead, nw), 0};
    if (ldsb::binE_size(nhead, nw) >= 4 * NB) b.islmin_off = ldsb::binE(NB, NP, hashed, capL);
    else if (capL >= NB) b.islmin_off = ldsb::con32(NB, NP, hashed, capL, 0);
    else { b.islmin_off = b.bytes; if (sleep) b.bytes += ldsb::A16(4 * NB); }
    return b;
}

// num_bots == 1024 with the full workgroup runs the fixed-size instantiation (compile-time LDS layout; without objects
// the contact capacity is a compile-time constant of the kernel, and the fixed-size instantiations with objects carry no
// sleep state)
constexpr bool fixed_1024(const PlanInput &in, int cap, int threads) {
    if (in.allow_sleep && in.num_objects > 0) return false;
    return in.drive_mode == KB_DRIVE_VELOCITY && in.num_bots == 1024 && in.light_type == KB_LIGHT_NONE && threads == 64 * MAX_WAVES &&
           BPT * 64 * MAX_WAVES == 1024 && (in.num_objects > 0 || cap == 4 * 1024 + 64);
}

inline Plan plan_launch(const PlanInput &in) {
    Plan r{};
    const int N = in.num_bots, M = in.num_objects;
    const bool mixed = in.drive_mode == KB_DRIVE_MIXED;
    const bool bins = M == 0 && !mixed;         // the sorted-bin image (namespace ldsb), else namespace lds
    const int NP = (N + 3) & ~3, NB = NP + KB_MAX_OBJECTS + 4, nmc = mc_candidates(in.num_fixtures);
    auto fail = [&](int status, const char *msg) { r.status = status; r.msg = msg; return r; };
    if (N > BPT * 64 * MAX_WAVES) return fail(KB_EINVAL, "kb_create: num_bots exceeds bots-per-thread x workgroup size of this build");

    // sparse swarms: a hash table of the cells instead of one list head per cell (kb_step_kernel.h, `hashed`); only where
    // it at least halves the table, and never for the fixed-size kernel
    int H = 64;
    while (H < 2 * N) H <<= 1;
    if (2 * H <= in.ncell && N != 1024) { r.nhead = H; r.hmask = H - 1; }
    else { r.nhead = in.ncell; r.hmask = 0; }

    long cap = (long)N * (N - 1) / 2 + 4L * N;
    if (cap > 2304) cap = 2304;
    if (cap < 4L * N + 64) cap = 4L * N + 64;
    cap += 40L * M;
    if (in.contact_capacity > 0) cap = in.contact_capacity;
    r.cap = (int)((cap + 7) & ~7L);

    // staging entries at `threads`: the fixed-size kernel without objects has its own
    auto staged = [&](int threads, int capL) { return bins && fixed_1024(in, r.cap, threads) ? ldsb::CAPL : capL; };
    auto image = [&](int threads, int capL) {
        const int nw = threads / 64;
        if (bins) return bins_image(NB, NP, r.hmask != 0, staged(threads, capL), r.nhead, nw, in.allow_sleep).bytes;
        return lds::total(lds::fixed(true, nw), NB, capL, NP, r.nhead, nmc);
    };
    // KB_DRIVE_MIXED: the drive law of every kilobot (one byte each) lies behind the image (Params.botlaw_off)
    auto bytes = [&](int threads, int capL) { return mixed ? lds::A16(image(threads, capL)) + lds::A16(NP) : image(threads, capL); };

    // with objects the LDS staging area gives up a few entries to the manifold-constraint records, so that two envs
    // of 1024 kilobots still share a CU
    int capLmax = M > 0 ? CAP_LDS - 8 * mc_candidates(in.num_fixtures) : CAP_LDS;
    // small swarms: stage what a packed cluster can produce (a hexagonal packing has < 3 contacts per kilobot, + walls) rather than all pairs, so
    // that more one-wave envs fit a CU; a spawn that overlaps more than that takes the global staging slice
    const int typical = 3 * N + 64 > 256 ? 3 * N + 64 : 256;
    if (capLmax > typical) capLmax = typical;
    int capL = r.cap < capLmax ? r.cap : capLmax;
    // sorted-bin image: scratch arrays of the sort lie over the staging area (2 B per kilobot over 4 B per entry); a
    // smaller contact_capacity still bounds what is staged (kernel: min(capL, cap)).  Kernels with objects: the per-island
    // minimum of the sleep times (N + M words) lies over the pair and info arrays of the LDS staging area, whatever
    // contact_capacity says
    int lo = bins ? ((NP / 2) + 7) & ~7 : ((NB + 1) / 2 + 7) & ~7;
    if (lo < 64) lo = 64;
    if (capL < lo) capL = lo;

    // Workgroup size (measured on MI355X, 64 ... 1024 kilobots): one kilobot per thread and a power-of-two wave count
    // (3 / 5 / 6 / 7-wave workgroups spread unevenly over the four SIMDs and lose a resident env), unless that costs
    // a resident env (LDS fit vs 16 waves per CU) while many lanes would idle.
    int T = 64;
    while (T < N && T < 64 * MAX_WAVES) T <<= 1;
    const int ldsT = bytes(T, capL), resident = M == 0 ? resident_envs_best(ldsT, T) : resident_envs(ldsT, T, KB_MIN_WAVES_PER_SIMD);
    if (T > 64 && resident < LDS_CU / ldsT && N * 100 < T * 85) T >>= 1;
    // 257 ... 512 kilobots without objects: two per thread in a 4-wave workgroup (measured at 512: 1.06e10 against 9.3e9 with
    // eight waves -- an 8-wave env takes a third of the CU's wave slots whatever its LDS image is)
    if (bins && N > 256 && N <= 512) T = 256;
    // with objects, up to 128 kilobots run as one wave: that selects the spill-free 256-VGPR instantiation
    // (kb_step), measured + 6 ... 9 % at 100 kilobots and - 3 % at 128 against two-wave workgroups
    if (M > 0 && N <= BPT * 64) T = 64;
    if (mixed) T = N <= BPT * 64 ? 64 : 64 * MAX_WAVES;       // the two spill-free instantiations (256 VGPRs)

    // The staging area is sized at this default width, whatever width is asked for.
    if (bins) {
        // sorted-bin image (16 B per staged contact): give up staging entries where that lets the CU hold one more env -- a
        // swarm of more than 512 kilobots down to the 688 of the fixed-size kernel (a settled swarm has ~ 0.55 contacts per
        // kilobot; a jammed one is staged in the global slice whatever the LDS holds, and what it needs is resident envs)
        // (smaller swarms: never below one contact per kilobot + 64 -- a settled lattice has ~ 0.5, a hexagonal cluster up to 3;
        //  the largest staging area that reaches the best residency is taken)
        const int least = N > 512 ? ldsb::CAPL : (N + 64 > 128 ? (N + 64 + 7) & ~7 : 128);
        int best = resident_envs_best(bytes(T, capL), T), bestc = capL;
        for (int c = capL - 8; c >= least; c -= 8)
            if (resident_envs_best(bytes(T, c), T) > best) { best = resident_envs_best(bytes(T, c), T); bestc = c; }
        capL = bestc;
    } else {   // trade a few staging entries for one more env per CU when the LDS footprint is just above a divisor of 160 KiB
        const int fit = LDS_CU / bytes(T, capL);
        const int least = 5 * N / 2 + 64 > 256 ? 5 * N / 2 + 64 : 256;
        int c = capL;
        while (c - 8 >= least && bytes(T, c) > LDS_CU / (fit + 1)) c -= 8;
        if (fit >= 1 && bytes(T, c) <= LDS_CU / (fit + 1)) capL = c;
    }

    if (in.threads) {           // kb_set_block_threads
        T = in.threads;
        if (T < 64 || T > 64 * MAX_WAVES || (T & 63)) return fail(KB_EINVAL, "kb_set_block_threads: multiple of 64 up to the build maximum");
        if (N > BPT * T) return fail(KB_EINVAL, "kb_set_block_threads: need num_bots <= bots-per-thread x threads");
    }
    r.threads = T;
    r.capL = staged(T, capL);
    r.lds_total = bytes(T, r.capL);
    r.islmin_off = bins_image(NB, NP, r.hmask != 0, r.capL, r.nhead, T / 64, in.allow_sleep).islmin_off;   // (only BINS kernels read it)
    r.botlaw_off = lds::A16(image(T, r.capL));
    r.tier = bins ? compact_tier(r.lds_total, T) : 0;
    if (r.lds_total > LDS_CU)
        return fail(KB_ELDS, in.threads ? "kb_set_block_threads: more than 160 KiB of LDS per env at this workgroup size"
                                        : "kb_create: configuration needs more than 160 KiB of LDS per env");
    if (in.threads && mixed && T != 64 && T != 64 * MAX_WAVES)
        return fail(KB_EINVAL, "kb_set_block_threads: KB_DRIVE_MIXED runs as one-wave or full workgroups");
    r.variant = select_variant({in.drive_mode, in.light_type, M > 0, in.all_discs, in.sense, in.allow_sleep, T, r.tier,
                                fixed_1024(in, r.cap, T)});
    r.status = KB_OK;
    return r;
}

}  // namespace kb
