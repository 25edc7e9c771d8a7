// kb_sense.h -- the kernels that sense on the current poses without stepping (kb_sense, kb_sense_neighbors,
// kb_sense_histogram, kb_sense_reduce, kb_sense_rays, kb_sense_edges): one workgroup per env, poses and the cell lists of the broadphase grid in LDS;
// kb_sense_objects, which meets objects and walls instead of kilobots and needs no cell lists; kb_sense_grid, which bins
// a whole env into an image of the table for an observer outside it; kb_sense_contacts, which reads no poses at all but
// the contact store the last step left; and kb_render, which draws every env as an RGB frame, a range query per pixel.
// Each kernel's LDS image is defined once, in the struct in front of it: the kernel takes its pointers from it, the entry
// point (kb_abi.hip) the dynamic-LDS size.  Included by kb_abi.hip only.
#pragma once

#include "kb_common.h"

namespace kb {

// The cell lists of the broadphase grid off the poses of one env in global memory: pos[b] and cellOf[b] of every kilobot
// (cell indices clamp to the grid), head[cell] -> nextb chains (plain heads: no hash).  o: index of the env's first kilobot.
// The order inside a chain is the order of the exchanges; nothing that reads the lists may depend on it.  Ends on a barrier.
__device__ __forceinline__ void kb_build_cell_lists(const Params &p, size_t o, float2 *pos, unsigned short *head,
                                                    unsigned short *nextb, unsigned short *cellOf, int tid, int nt) {
    for (int c = tid; c < p.ncell; c += nt) head[c] = EMPTY16;
    __syncthreads();
    for (int b = tid; b < p.N; b += nt) {
        const float bx = p.buf.x[o + b], by = p.buf.y[o + b];
        pos[b].x = bx; pos[b].y = by;
        int cx = (int)floorf((bx - p.xmin) * p.inv_cell);
        int cy = (int)floorf((by - p.ymin) * p.inv_cell);
        cx = cx < 0 ? 0 : (cx >= p.gw ? p.gw - 1 : cx);
        cy = cy < 0 ? 0 : (cy >= p.gh ? p.gh - 1 : cy);
        const int cell = cy * p.gw + cx;
        cellOf[b] = (unsigned short)cell;
        nextb[b] = (unsigned short)kb_exch16(head, cell, (unsigned)b);
    }
    __syncthreads();
}

// The full-stencil walk of kilobot a (in `cell`, at pa): every cell within reach s of its own, eight list heads per LDS
// round trip (most cells are empty), down each chain.  Calls hit(b, ex, ey, dd) for every kilobot b != a with !(dd > R2),
// (ex, ey) = pos[b] - pa, dd = ex^2 + ey^2, and returns how many there were.  (The half stencil of kb_sense_pass meets every
// pair once and counts with atomics: a different traversal.)  hit is taken by value: taken by reference, the 16-slot list
// kernel needed 156 VGPRs instead of 130 and ran 4 % slower.
template <typename Hit>
__device__ __forceinline__ unsigned kb_walk_in_range(const Params &p, const float2 *pos, const unsigned short *head,
                                                     const unsigned short *nextb, const int a, const int cell, const float2 pa,
                                                     const int s, const float R2, Hit hit) {
    constexpr int W = 8;
    const int cx = cell % p.gw, cy = cell / p.gw;
    unsigned cnt = 0;
    const int y1 = min(cy + s, p.gh - 1), x0 = max(cx - s, 0), x1 = min(cx + s, p.gw - 1);
    for (int oy = max(cy - s, 0); oy <= y1; ++oy) {
        for (int xb = x0; xb <= x1; xb += W) {
            unsigned cur[W];
#pragma unroll
            for (int i = 0; i < W; ++i) cur[i] = xb + i <= x1 ? (unsigned)head[oy * p.gw + xb + i] : (unsigned)EMPTY16;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                for (unsigned b = cur[i]; b != (unsigned)EMPTY16;) {
                    const float2 pb = pos[b];
                    const unsigned nb = nextb[b];
                    const float ex = pb.x - pa.x, ey = pb.y - pa.y;
                    const float dd = ex * ex + ey * ey;
                    if ((int)b != a && !(dd > R2)) {
                        cnt++;
                        hit(b, ex, ey, dd);
                    }
                    b = nb;
                }
            }
        }
    }
    return cnt;
}

// ---- kb_sense: counts --------------------------------------------------------------------------------------------------
struct SenseLds {       // byte offsets: pos (float2) at 0, the packed u16 counters, nextb, cellOf, head (u16 each)
    int cnt16, nextb, cellOf, head, bytes;
    __host__ __device__ constexpr SenseLds(int NP, int ncell)
        : cnt16(8 * NP), nextb(10 * NP), cellOf(12 * NP), head(14 * NP), bytes(14 * NP + 2 * ncell + 16) {}
};

// IR-range neighbour sensing on the current poses (kb_sense): the sensing pass of the step kernel on the cell lists
__global__ void __launch_bounds__(256) kb_sense_kernel(const Params p, const int s, const float R2, unsigned *out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, N = p.N;
    const SenseLds L(p.NP, p.ncell);
    float2 *pos = reinterpret_cast<float2 *>(smem);
    unsigned *cnt16 = reinterpret_cast<unsigned *>(smem + L.cnt16);
    unsigned short *nextb = reinterpret_cast<unsigned short *>(smem + L.nextb);
    unsigned short *cellOf = reinterpret_cast<unsigned short *>(smem + L.cellOf);
    unsigned short *head = reinterpret_cast<unsigned short *>(smem + L.head);
    const size_t o = (size_t)e * N;
    for (int b = tid; b < p.NP / 2; b += nt) cnt16[b] = 0;
    kb_build_cell_lists(p, o, pos, head, nextb, cellOf, tid, nt);
    kb_sense_pass(pos, head, nextb, cellOf, cnt16, N, nt, tid, p.gw, p.gh, s, R2, 0);
    __syncthreads();
    for (int b = tid; b < N; b += nt) out[o + b] = (unsigned)reinterpret_cast<unsigned short *>(cnt16)[b];
}

// ---- kb_sense_neighbors: the k nearest ---------------------------------------------------------------------------------
struct NeighborsLds {   // byte offsets: pos (float2) at 0, th (float), nextb, cellOf, head (u16 each)
    int th, nextb, cellOf, head, bytes;
    __host__ __device__ constexpr NeighborsLds(int NP, int ncell)
        : th(8 * NP), nextb(12 * NP), cellOf(14 * NP), head(16 * NP), bytes(16 * NP + 2 * ncell + 16) {}
};

// Nearest-neighbour lists with body-frame offsets on the current poses (kb_sense_neighbors): poses, headings and the cell
// lists in LDS, one kilobot per lane.  Every kilobot walks the FULL stencil of reach s (it needs its own ordered list, so the
// half-stencil trick of kb_sense_pass does not apply) and keeps the K best keys (bits of d2) << 32 | j in registers:
// d2 >= 0, so the unsigned order of the key is the order by (d2, j).  A candidate in range that beats the worst kept key
// runs down an unrolled compare-exchange chain (best[] stays sorted; every index is a compile-time constant, so best[]
// never leaves the registers).  K: the requested k rounded up to 4, 8 or 16.
// Rows are written per lane: slot i of kilobot a is one 16-byte store, its k slots are contiguous.
template <int K>
__global__ void __launch_bounds__(256) kb_neighbors_kernel(const Params p, const int s, const float R2, const int k, const int vec,
                                                           int *d_index, float4 *d_rel, unsigned *d_count) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr unsigned long long NONE = ~0ull;
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, N = p.N;
    const NeighborsLds L(p.NP, p.ncell);
    float2 *pos = reinterpret_cast<float2 *>(smem);
    float *th = reinterpret_cast<float *>(smem + L.th);
    unsigned short *nextb = reinterpret_cast<unsigned short *>(smem + L.nextb);
    unsigned short *cellOf = reinterpret_cast<unsigned short *>(smem + L.cellOf);
    unsigned short *head = reinterpret_cast<unsigned short *>(smem + L.head);
    const size_t o = (size_t)e * N;
    for (int b = tid; b < N; b += nt) th[b] = p.buf.theta[o + b];
    kb_build_cell_lists(p, o, pos, head, nextb, cellOf, tid, nt);
    for (int a = tid; a < N; a += nt) {
        const int cell = cellOf[a];
        const float2 pa = pos[a];
        unsigned long long best[K];
#pragma unroll
        for (int i = 0; i < K; ++i) best[i] = NONE;
        const unsigned cnt = kb_walk_in_range(p, pos, head, nextb, a, cell, pa, s, R2, [&](unsigned b, float, float, float dd) {
            unsigned long long key = ((unsigned long long)__float_as_uint(dd) << 32) | b;
            if (key < best[K - 1]) {
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    const unsigned long long lo = key < best[q] ? key : best[q];
                    key = key < best[q] ? best[q] : key;
                    best[q] = lo;
                }
            }
        });
        const float tha = th[a];
        float sn, cs;
        kb_sincosf(tha, sn, cs);
        const size_t row = (o + a) * (size_t)k;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (i >= k) break;
            const bool used = best[i] != NONE;
            const unsigned j = used ? (unsigned)best[i] : (unsigned)a;
            const float2 pb = pos[j];
            const float ex = pb.x - pa.x, ey = pb.y - pa.y;
            const float d2 = __uint_as_float((unsigned)(best[i] >> 32));
            float4 r;
            r.x = (cs * ex + sn * ey) / WORLD_SCALE;
            r.y = (cs * ey - sn * ex) / WORLD_SCALE;
            r.z = sqrtf(d2) / WORLD_SCALE;
            r.w = th[j] - tha;
            if (!used) r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            d_rel[row + i] = r;
        }
        if (vec) {      // k is a multiple of 4 and d_index is 16-byte aligned: four indices per store
#pragma unroll
            for (int i = 0; i < K; i += 4) {
                if (i >= k) break;
                int4 v;
                v.x = (int)(unsigned)best[i]; v.y = (int)(unsigned)best[i + 1]; v.z = (int)(unsigned)best[i + 2]; v.w = (int)(unsigned)best[i + 3];
                reinterpret_cast<int4 *>(d_index + row)[i >> 2] = v;      // (the low word of NONE is -1)
            }
        } else {
#pragma unroll
            for (int i = 0; i < K; ++i) {
                if (i >= k) break;
                d_index[row + i] = (int)(unsigned)best[i];
            }
        }
        if (d_count) d_count[o + a] = cnt;
    }
}

// ---- kb_sense_histogram: ring x sector counts --------------------------------------------------------------------------
struct HistArgs {
    int n_rings, n_sectors;
    float e2[KB_HIST_MAX_RINGS - 1];            // E2_r of ring edge r + 1
    float ux[KB_HIST_MAX_SECTORS / 2 - 1];      // u_m of sector boundary m + 1 (kb_histogram_sectors)
    float uy[KB_HIST_MAX_SECTORS / 2 - 1];
};
constexpr int HIST_TILE = 256;
constexpr int HIST_STRIDE = HIST_TILE + 2;
constexpr int HIST_TABLE_BYTES = 4 * (KB_HIST_MAX_RINGS + KB_HIST_MAX_SECTORS - 3);

struct HistLds {        // byte offsets: pos (float2) at 0, nextb, cellOf, head, hist[bins][HIST_STRIDE] (u16 each), tab (float)
    int nextb, cellOf, head, hist, tab, bytes;
    __host__ __device__ constexpr HistLds(int NP, int ncell, int bins)
        : nextb(8 * NP), cellOf(10 * NP), head(12 * NP),
          hist(head + 2 * ((ncell + 1) & ~1)),      // (kb_exch16 works on whole words of head)
          tab(hist + 2 * bins * HIST_STRIDE), bytes(tab + HIST_TABLE_BYTES) {}
};
// the largest image (1024 kilobots, every cell, 64 bins) stays under the default limit for dynamic LDS: no attribute to raise
static_assert(HistLds(KB_MAX_BOTS, MAX_CELLS, KB_HIST_MAX_BINS).bytes <= 64 * 1024, "kb_histogram_kernel: LDS image");

// Local neighbour histograms on the current poses (kb_sense_histogram): every kilobot counts ALL kilobots of its env in IR
// range, binned by ring (distance) and sector (bearing in its own frame).  Poses and the cell lists in LDS, one kilobot per
// lane over the full stencil.  A kilobot's heading is used once, by its own lane, so it is read straight from global
// memory into a register.
// Accumulator: the env is processed in tiles of 256 kilobots; lane t owns column t of u16 hist[bin][HIST_STRIDE] in LDS
// (a count is at most N - 1 <= 1023) and is the only one to update it: no atomics, no per-lane array, no scratch.  After
// the tile's walk and a barrier the workgroup writes the tile's n * B floats with the flat index f = tid + 256 i
// (kilobot f / B, bin f % B, both kept incrementally): consecutive lanes store consecutive floats.  HIST_STRIDE = 258
// halfwords = 129 words: in that read-out the lanes of a wave read bins of one or two kilobots, and the odd word stride
// puts them on different banks (a stride of 256 would put all 64 on one).  The edge and boundary tables arrive as a kernel
// argument and go through LDS into per-lane registers, and the ring and sector counts run over the whole tables without
// branches (unused edges are +inf, unused boundaries (0, 0): they count nothing): with the tables in SGPRs next to Params,
// or with a uniform early exit per table entry, the kernel spilled SGPRs.
__global__ void __launch_bounds__(256) kb_histogram_kernel(const Params p, const int s, const float R2, const HistArgs h,
                                                           float *d_hist, unsigned *d_count) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int NE = KB_HIST_MAX_RINGS - 1, NU = KB_HIST_MAX_SECTORS / 2 - 1;
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, N = p.N;
    const int B = h.n_rings * h.n_sectors, H = h.n_sectors >> 1;
    const HistLds L(p.NP, p.ncell, B);
    float2 *pos = reinterpret_cast<float2 *>(smem);
    unsigned short *nextb = reinterpret_cast<unsigned short *>(smem + L.nextb);
    unsigned short *cellOf = reinterpret_cast<unsigned short *>(smem + L.cellOf);
    unsigned short *head = reinterpret_cast<unsigned short *>(smem + L.head);
    unsigned short *hist = reinterpret_cast<unsigned short *>(smem + L.hist);
    float *tab = reinterpret_cast<float *>(smem + L.tab);
    const size_t o = (size_t)e * N;
    if (tid == 0) {
#pragma unroll
        for (int r = 0; r < NE; ++r) tab[r] = h.e2[r];
#pragma unroll
        for (int m = 0; m < NU; ++m) { tab[NE + m] = h.ux[m]; tab[NE + NU + m] = h.uy[m]; }
    }
    kb_build_cell_lists(p, o, pos, head, nextb, cellOf, tid, nt);
    float e2[NE], ux[NU], uy[NU];
#pragma unroll
    for (int r = 0; r < NE; ++r) e2[r] = tab[r];
#pragma unroll
    for (int m = 0; m < NU; ++m) { ux[m] = tab[NE + m]; uy[m] = tab[NE + NU + m]; }
    const int q256 = HIST_TILE / B, r256 = HIST_TILE % B;
    for (int t0 = 0; t0 < N; t0 += HIST_TILE) {
        const int a = t0 + tid;
        unsigned short *col = hist + tid;
        for (int b = 0; b < B; ++b) col[b * HIST_STRIDE] = 0;
        if (a < N) {
            const int cell = cellOf[a];
            const float2 pa = pos[a];
            float sn, cs;
            kb_sincosf(p.buf.theta[o + a], sn, cs);
            const unsigned cnt = kb_walk_in_range(p, pos, head, nextb, a, cell, pa, s, R2, [&](unsigned, float ex, float ey, float dd) {
                int ring = 0;
#pragma unroll
                for (int r = 0; r < NE; ++r) ring += dd > e2[r] ? 1 : 0;
                int sector = 0;
                if (H > 0) {
                    float ah = cs * ex + sn * ey;
                    float lf = cs * ey - sn * ex;
                    const bool low = lf < 0.0f;
                    if (low) { ah = -ah; lf = -lf; }
#pragma unroll
                    for (int m = 0; m < NU; ++m) sector += ux[m] * lf - uy[m] * ah > 0.0f ? 1 : 0;
                    sector += low ? H : 0;      // (a select: as `if (low)` it became a branch, + 1 % on the launch)
                }
                unsigned short *c = col + (ring * h.n_sectors + sector) * HIST_STRIDE;
                *c = (unsigned short)(*c + 1u);
            });
            if (d_count) d_count[o + a] = cnt;
        }
        __syncthreads();
        const int total = min(HIST_TILE, N - t0) * B;
        float *out = d_hist + (o + t0) * (size_t)B;
        int kb = tid / B, bin = tid % B;
        for (int f = tid; f < total; f += HIST_TILE) {
            out[f] = (float)hist[bin * HIST_STRIDE + kb];
            kb += q256; bin += r256;
            if (bin >= B) { bin -= B; kb++; }
        }
        __syncthreads();
    }
}

// ---- kb_sense_reduce: the messages of the kilobots in range, summed or ordered -----------------------------------------
struct ReduceLds {      // byte offsets: pos (float2) at 0, nextb, cellOf, head (u16 each), msg[NP][CP] (one 32-bit word per channel)
    int nextb, cellOf, head, msg, bytes;
    __host__ __device__ constexpr ReduceLds(int NP, int ncell, int CP)
        : nextb(8 * NP), cellOf(10 * NP), head(12 * NP),
          msg((head + 2 * ((ncell + 1) & ~1) + 15) & ~15),      // (rows are read 4, 8 or 16 bytes at a time)
          bytes(msg + 4 * CP * NP) {}
};
// the largest image (1024 kilobots, every cell, 8 channels) stays under the default limit for dynamic LDS: no attribute to raise
static_assert(ReduceLds(KB_MAX_BOTS, MAX_CELLS, KB_REDUCE_MAX_CHANNELS).bytes <= 64 * 1024, "kb_reduce_kernel: LDS image");

// The total order of the bit patterns as unsigned keys: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.
__device__ __forceinline__ unsigned kb_reduce_key(unsigned bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ unsigned kb_reduce_unkey(unsigned key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
// The fixed-point image of a broadcast value: NaN -> 0, otherwise v * scale clamped to +-2^21 and rounded half to even.
__device__ __forceinline__ int kb_reduce_quant(float v, float scale) {
    const float t = v * scale;
    return t != t ? 0 : (int)rintf(fminf(fmaxf(t, -2097152.0f), 2097152.0f));
}

// IR-range message aggregation on the current poses (kb_sense_reduce): every kilobot combines, channel by channel, what the
// kilobots of its env in IR range broadcast.  Poses and the cell lists in LDS, one kilobot per lane over the full stencil,
// like kb_neighbors_kernel.  Every broadcast value is converted ONCE, while the env is staged: to its fixed-point int32 for
// the sum, to its order key for min / max, so that LDS holds one 32-bit word per (kilobot, channel) in rows of CP words
// (the channels rounded up to 1, 2, 4 or 8: one LDS read of 4, 8 or 16 bytes, two of 16 for CP = 8, fetches a neighbour's
// whole message) and the work per pair is an integer add, unsigned min or unsigned max per channel into CP per-lane
// registers.  No two floats are ever added: the result does not depend on the order of the chains.  The words go back to
// floats once per kilobot, at write-out: one row of C floats per lane, in 16-byte stores with vec (C a multiple of 4 and
// d_out 16-byte aligned).  Padding channels hold the identity and are never written.  d_out may be d_values: the env's
// values are all in LDS before the barrier that ends kb_build_cell_lists, and nothing is written before it.
template <int OP, int CP>
__global__ void __launch_bounds__(256) kb_reduce_kernel(const Params p, const int s, const float R2, const int C, const int vec,
                                                        const float scale, const float *d_values, float *d_out, unsigned *d_count) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr unsigned IDENT = OP == KB_REDUCE_MIN ? 0xFFFFFFFFu : 0u;      // of the words: sum 0, min the top key, max the bottom key
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, N = p.N;
    const ReduceLds L(p.NP, p.ncell, CP);
    float2 *pos = reinterpret_cast<float2 *>(smem);
    unsigned short *nextb = reinterpret_cast<unsigned short *>(smem + L.nextb);
    unsigned short *cellOf = reinterpret_cast<unsigned short *>(smem + L.cellOf);
    unsigned short *head = reinterpret_cast<unsigned short *>(smem + L.head);
    unsigned *msg = reinterpret_cast<unsigned *>(smem + L.msg);
    const size_t o = (size_t)e * N;
    const float *val = d_values + o * (size_t)C;
    for (int f = tid; f < N * CP; f += nt) {
        const int b = f / CP, c = f % CP;
        unsigned w = IDENT;
        if (c < C) {
            const float v = val[b * C + c];
            w = OP == KB_REDUCE_SUM ? (unsigned)kb_reduce_quant(v, scale) : kb_reduce_key(__float_as_uint(v));
        }
        msg[f] = w;
    }
    kb_build_cell_lists(p, o, pos, head, nextb, cellOf, tid, nt);
    for (int a = tid; a < N; a += nt) {
        const int cell = cellOf[a];
        const float2 pa = pos[a];
        unsigned acc[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) acc[c] = IDENT;
        const unsigned cnt = kb_walk_in_range(p, pos, head, nextb, a, cell, pa, s, R2, [&](unsigned b, float, float, float) {
            unsigned w[CP];
            if constexpr (CP == 1) {
                w[0] = msg[b];
            } else if constexpr (CP == 2) {
                const uint2 r = reinterpret_cast<const uint2 *>(msg)[b];
                w[0] = r.x; w[1] = r.y;
            } else {
#pragma unroll
                for (int q = 0; q < CP / 4; ++q) {
                    const uint4 r = reinterpret_cast<const uint4 *>(msg)[b * (CP / 4) + q];
                    w[4 * q] = r.x; w[4 * q + 1] = r.y; w[4 * q + 2] = r.z; w[4 * q + 3] = r.w;
                }
            }
#pragma unroll
            for (int c = 0; c < CP; ++c)
                acc[c] = OP == KB_REDUCE_SUM ? acc[c] + w[c] : OP == KB_REDUCE_MIN ? min(acc[c], w[c]) : max(acc[c], w[c]);
        });
        float r[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            if (OP == KB_REDUCE_SUM) r[c] = (float)(int)acc[c] / scale;
            else r[c] = __uint_as_float(cnt ? kb_reduce_unkey(acc[c]) : OP == KB_REDUCE_MIN ? 0x7F800000u : 0xFF800000u);   // nothing heard: +inf / -inf
        }
        float *row = d_out + (o + a) * (size_t)C;
        if (CP >= 4 && vec) {       // C == CP and d_out is 16-byte aligned: four channels per store
#pragma unroll
            for (int c = 0; c + 3 < CP; c += 4) reinterpret_cast<float4 *>(row)[c >> 2] = make_float4(r[c], r[c + 1], r[c + 2], r[c + 3]);
        } else {
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                if (c >= C) break;
                row[c] = r[c];
            }
        }
        if (d_count) d_count[o + a] = cnt;
    }
}

// ---- kb_sense_objects: the nearest point of every object and of the walls ------------------------------------------------
#ifndef KB_OBJECTS_TILE
#define KB_OBJECTS_TILE 256             // kilobots (= lanes) per workgroup of kb_objects_kernel: a multiple of 64 up to 256 (A/B knob)
#endif
constexpr int OBJ_TILE = KB_OBJECTS_TILE;
static_assert(OBJ_TILE % 64 == 0 && OBJ_TILE >= 64 && OBJ_TILE <= 256, "kb_objects_kernel: tile");
constexpr int OBJ_EDGES = KB_MAX_OBJECTS * KB_MAX_POLY_VERTS;
struct ObjectsLds {     // byte offsets: frame[M] (float4: ox, oy, sin, cos) at 0, edge[F][4][2] (float4 pairs), fix[F] (nverts, radius), first[M + 1]
    int edge, fix, first, bytes;
    __host__ __device__ constexpr ObjectsLds()
        : edge(16 * KB_MAX_OBJECTS), fix(edge + 32 * OBJ_EDGES), first(fix + 8 * KB_MAX_OBJECTS), bytes(first + 16 * ((KB_MAX_OBJECTS + 4) / 4)) {}
};

// Pointers into the LDS image of ObjectsLds
struct ObjectsImage {
    float4 *frame, *edge;
    float2 *fix;
    int *first;
    __device__ __forceinline__ explicit ObjectsImage(unsigned char *smem) {
        constexpr ObjectsLds L;
        frame = reinterpret_cast<float4 *>(smem);
        edge = reinterpret_cast<float4 *>(smem + L.edge);
        fix = reinterpret_cast<float2 *>(smem + L.fix);
        first = reinterpret_cast<int *>(smem + L.first);
    }
};

// Once per workgroup (of at least 64 lanes) the object frames of env e (ox, oy, sin, cos: one kb_sincosf in each of the
// first M lanes) and the fixture table go to LDS.  The table (kb_outline, fixtures grouped by body on the host) arrives as a
// kernel argument and is staged edge by edge: lane 4 f + k stores a, e = b - a and e . e of edge k of fixture f -- values
// every lane would otherwise compute for itself, each a single fp32 operation and therefore the same bits whoever evaluates
// it.  Lane m stores first[m], the number of fixtures of lower bodies: object m's fixtures are first[m] .. first[m + 1] - 1.
// Ends on a barrier.
__device__ __forceinline__ void kb_stage_objects(const kb_outline &ol, const ObjectsImage &I, const int e, const int tid,
                                                 const float *ox, const float *oy, const float *otheta) {
    const int M = ol.num_objects, F = ol.num_fixtures;
    if (tid < M) {
        const size_t j = (size_t)e * M + tid;
        float so, co;
        kb_sincosf(otheta[j], so, co);
        I.frame[tid] = make_float4(ox[j], oy[j], so, co);
    }
    if (tid < OBJ_EDGES) {
        const int f = tid / KB_MAX_POLY_VERTS, k = tid % KB_MAX_POLY_VERTS;
        const int n = f < F ? ol.nverts[f] : 0;
        if (k < n) {
            const int k1 = k + 1 == n ? 0 : k + 1;
            const float ax = ol.verts[f][k][0], ay = ol.verts[f][k][1], bx = ol.verts[f][k1][0], by = ol.verts[f][k1][1];
            const float ex = bx - ax, ey = by - ay;
            I.edge[2 * tid] = make_float4(ax, ay, ex, ey);
            I.edge[2 * tid + 1] = make_float4(bx, by, ex * ex + ey * ey, 0.0f);
        }
        if (k == 0 && f < F) I.fix[f] = make_float2(__int_as_float(n), ol.radius[f]);
    }
    if (tid <= M) {
        int c = 0;
        for (int f = 0; f < F; ++f) c += ol.body[f] < tid ? 1 : 0;
        I.first[tid] = c;
    }
    __syncthreads();
}

// The point (xi, yi) against object m of the staged env, fixtures -> edges with the running best candidate in scalars and
// all table reads from LDS at addresses that are the same in every lane (broadcasts): returns the inside flag (the point is
// covered by ANY fixture of the object: cr >= 0 on all edges of a polygon, !(g > 0) for a circle) and leaves the nearest
// candidate in best (d2) and (brx, bry) (object frame).  The ONE definition of the predicate, for kb_objects_kernel and
// kb_grid_objects_kernel; a caller that drops best, brx and bry leaves their arithmetic to dead-code elimination.  The loop
// bounds are the same in all lanes and are made scalar with readfirstlane.
__device__ __forceinline__ bool kb_object_walk(const ObjectsImage &I, const int m, const float4 fr, const float xi, const float yi,
                                               float &best, float &brx, float &bry) {
    const float so = fr.z, co = fr.w;
    const float dx = xi - fr.x, dy = yi - fr.y;
    const float px = co * dx + so * dy, py = co * dy - so * dx;
    best = INFINITY; brx = 0.0f; bry = 0.0f;
    bool inside = false;
    const int f0 = __builtin_amdgcn_readfirstlane(I.first[m]), f1 = __builtin_amdgcn_readfirstlane(I.first[m + 1]);
    for (int f = f0; f < f1; ++f) {
        const float2 fx = I.fix[f];
        const int n = __builtin_amdgcn_readfirstlane(__float_as_int(fx.x));
        if (n == 0) {
            const float r = fx.y;
            const float n2 = px * px + py * py;
            const float nn = sqrtf(n2);
            const float g = nn - r;
            float rx = r, ry = 0.0f;
            if (nn > 0.0f) { rx = -(g * (px / nn)); ry = -(g * (py / nn)); }
            const float d2 = g * g;
            if (d2 < best) { best = d2; brx = rx; bry = ry; }
            inside = inside || !(g > 0.0f);
        } else {
            bool in_f = true;
            for (int k = 0; k < n; ++k) {
                const float4 ea = I.edge[2 * (KB_MAX_POLY_VERTS * f + k)], eb = I.edge[2 * (KB_MAX_POLY_VERTS * f + k) + 1];
                const float ex = ea.z, ey = ea.w;
                const float wx = px - ea.x, wy = py - ea.y;
                const float t = (wx * ex + wy * ey) / eb.z;
                float qx = ea.x + t * ex, qy = ea.y + t * ey;
                if (t >= 1.0f) { qx = eb.x; qy = eb.y; }
                if (!(t > 0.0f)) { qx = ea.x; qy = ea.y; }
                const float rx = qx - px, ry = qy - py;
                const float d2 = rx * rx + ry * ry;
                if (d2 < best) { best = d2; brx = rx; bry = ry; }
                in_f = in_f && ex * wy - ey * wx >= 0.0f;
            }
            inside = inside || in_f;
        }
    }
    return inside;
}

// Object and wall points on the current poses (kb_sense_objects): one kilobot per lane, workgroups over (env, tile of
// kilobots); no stencil and no cell lists, every kilobot meets every fixture of its env.  Once per workgroup the env's
// object frames and the fixture table go to LDS (kb_stage_objects); then every lane runs objects -> fixtures -> edges
// (kb_object_walk): no per-object register array is ever indexed by a run-time number, nothing goes to scratch.  A lane
// writes the M consecutive rows of its own kilobot, one 16-byte store each (the layout kb_neighbors_kernel uses for its
// slots), then the wall row.
__global__ void __launch_bounds__(OBJ_TILE) kb_objects_kernel(const kb_outline ol, const int N, const int tiles, const float *x, const float *y,
                                                         const float *theta, const float *ox, const float *oy, const float *otheta,
                                                         float4 *d_obj, float4 *d_wall) {
    extern __shared__ __align__(16) unsigned char smem[];
    const ObjectsImage I(smem);
    const int tid = threadIdx.x, e = blockIdx.x / tiles, a = (blockIdx.x % tiles) * blockDim.x + tid;
    const int M = ol.num_objects;
    if (d_obj) kb_stage_objects(ol, I, e, tid, ox, oy, otheta);
    if (a >= N) return;
    const size_t i = (size_t)e * N + a;
    const float xi = x[i], yi = y[i];
    float si, ci;
    kb_sincosf(theta[i], si, ci);
    if (d_obj) {
        float4 *row = d_obj + i * (size_t)M;
        for (int m = 0; m < M; ++m) {
            const float4 fr = I.frame[m];
            const float so = fr.z, co = fr.w;
            float best, brx, bry;
            const bool inside = kb_object_walk(I, m, fr, xi, yi, best, brx, bry);
            const float gx = co * brx - so * bry, gy = so * brx + co * bry;
            row[m] = make_float4((ci * gx + si * gy) / WORLD_SCALE, (ci * gy - si * gx) / WORLD_SCALE, sqrtf(best) / WORLD_SCALE, inside ? 1.0f : 0.0f);
        }
    }
    if (d_wall) {
        const float g0 = xi - ol.arena[0], g1 = ol.arena[1] - xi, g2 = yi - ol.arena[2], g3 = ol.arena[3] - yi;
        float g = g0, gx = -g0, gy = 0.0f, w = 0.0f;
        if (g1 < g) { g = g1; gx = g1; w = 1.0f; }
        if (g2 < g) { g = g2; gx = 0.0f; gy = -g2; w = 2.0f; }
        if (g3 < g) { g = g3; gx = 0.0f; gy = g3; w = 3.0f; }
        d_wall[i] = make_float4((ci * gx + si * gy) / WORLD_SCALE, (ci * gy - si * gx) / WORLD_SCALE, g / WORLD_SCALE, w);
    }
}

// ---- kb_sense_grid: top-down occupancy grids of every env ----------------------------------------------------------------
constexpr int GRID_LDS_LIMIT = 64 * 1024;       // the default limit for dynamic LDS: no attribute to raise
struct GridLds {        // the int32 counters of one band of rows, plane by plane: acc[words][rows][gw] (count, sum of qc, sum of qs)
    int bands, rows, plane, bytes;      // bands per env; rows per band (the last band may hold fewer); words per plane; the image
    static constexpr int max_rows(int gw, int words) { return GRID_LDS_LIMIT / (4 * words * gw); }
    // the fewest bands whose image stays within the limit, then rows spread evenly over them
    __host__ __device__ constexpr GridLds(int gw, int gh, int words)
        : bands((gh + max_rows(gw, words) - 1) / max_rows(gw, words)), rows((gh + bands - 1) / bands), plane(rows * gw), bytes(4 * words * plane) {}
};
static_assert(GridLds(64, 48, 3).bands == 1 && GridLds(64, 48, 3).bytes == 36 * 1024, "kb_grid_bots_kernel: one band of 36 KiB");
static_assert(GridLds(KB_GRID_MAX_SIDE, KB_GRID_MAX_SIDE, 3).bytes <= GRID_LDS_LIMIT && GridLds(KB_GRID_MAX_SIDE, KB_GRID_MAX_SIDE, 1).bytes <= GRID_LDS_LIMIT,
              "kb_grid_bots_kernel: LDS image");

// The kilobot planes of kb_sense_grid: one workgroup per (env, band of rows), the band's counters as int32 words in LDS.  The
// workgroup zeroes them, reads the env's x, y once (coalesced, up to four kilobots per lane; theta only with the flow and only
// of the kilobots of its band), bins every kilobot and adds those of its band into LDS with atomics whose result is not
// used (ds_add_u32: nothing comes back); all 1024 kilobots in one cell serialise on one word and stay correct.  After one
// barrier the planes go out as floats, consecutive lanes to consecutive words (the rows of a band are contiguous in a
// channel), 16 bytes per lane with vec (gw a multiple of 4 and d_out 16-byte aligned: every band of every channel then starts
// on 16 bytes, in LDS and in d_out).  Every output word is written exactly once, by a plain store: no global atomics, no
// cleared buffer.  No two floats are ever added: the flow is the integer sum of the fixed-point images of kb_reduce_quant.
// PL: KB_GRID_COUNT | KB_GRID_FLOW, the planes asked for; their channels are the first of the env's C.  bands, band_rows: of GridLds.
template <int PL>
__global__ void __launch_bounds__(256) kb_grid_bots_kernel(const int N, const int gw, const int gh, const int bands, const int band_rows, const int C,
                                                           const int vec, const float xmin, const float ymin, const float icw, const float ich,
                                                           const float *x, const float *y, const float *theta, float *d_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr bool COUNT = (PL & KB_GRID_COUNT) != 0, FLOW = (PL & KB_GRID_FLOW) != 0;
    constexpr int W = (COUNT ? 1 : 0) + (FLOW ? 2 : 0);
    static_assert(W > 0, "kb_grid_bots_kernel: no plane");
    const int tid = threadIdx.x, nt = blockDim.x, e = blockIdx.x / bands, row0 = (blockIdx.x % bands) * band_rows;
    const int rows = min(band_rows, gh - row0), plane = band_rows * gw;      // (GridLds: sized on the host)
    int *acc = reinterpret_cast<int *>(smem);
    for (int f = tid; f < W * plane; f += nt) acc[f] = 0;
    __syncthreads();
    const size_t o = (size_t)e * N;
    for (int b = tid; b < N; b += nt) {
        const float tx = (x[o + b] - xmin) * icw, ty = (y[o + b] - ymin) * ich;
        const int ix = !(tx > 0.0f) ? 0 : tx >= (float)gw ? gw - 1 : (int)tx;
        const int iy = !(ty > 0.0f) ? 0 : ty >= (float)gh ? gh - 1 : (int)ty;
        const int r = iy - row0;
        if (r < 0 || r >= rows) continue;
        int *c = acc + r * gw + ix;
        if (COUNT) {
            atomicAdd(c, 1);
            c += plane;
        }
        if (FLOW) {
            float sn, cs;
            kb_sincosf(theta[o + b], sn, cs);
            atomicAdd(c, kb_reduce_quant(cs, 65536.0f));
            atomicAdd(c + plane, kb_reduce_quant(sn, 65536.0f));
        }
    }
    __syncthreads();
    const size_t chan = (size_t)gh * gw;
    float *band = d_out + ((size_t)e * C * gh + row0) * gw;     // the band's first row in channel 0 of the env
    const int n = rows * gw;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const float div = COUNT && w == 0 ? 1.0f : 65536.0f;        // (a division by 1 is exact: the count is the float of the integer)
        const int *src = acc + w * plane;
        float *dst = band + w * chan;
        if (vec) {
            for (int f = tid; f < n / 4; f += nt) {
                const int4 v = reinterpret_cast<const int4 *>(src)[f];
                reinterpret_cast<float4 *>(dst)[f] = make_float4((float)v.x / div, (float)v.y / div, (float)v.z / div, (float)v.w / div);
            }
        } else {
            for (int f = tid; f < n; f += nt) dst[f] = (float)src[f] / div;
        }
    }
}

// The object planes of kb_sense_grid: one lane per cell, workgroups over (env, tile of cells); the env's object frames and the
// fixture table are staged as in kb_objects_kernel and every lane asks kb_object_walk whether its cell centre is covered,
// object by object.  Lanes of a wave hold consecutive cells: each object's store is one run of consecutive words.
// ch0: the first object channel among the env's C.
__global__ void __launch_bounds__(256) kb_grid_objects_kernel(const kb_outline ol, const int gw, const int gh, const int tiles, const int C, const int ch0,
                                                              const float cw, const float ch, const float *ox, const float *oy, const float *otheta,
                                                              float *d_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const ObjectsImage I(smem);
    const int tid = threadIdx.x, e = blockIdx.x / tiles, cell = (blockIdx.x % tiles) * blockDim.x + tid;
    const int M = ol.num_objects;
    kb_stage_objects(ol, I, e, tid, ox, oy, otheta);
    if (cell >= gw * gh) return;
    const int iy = cell / gw, ix = cell - iy * gw;
    const float cx = ol.arena[0] + ((float)ix + 0.5f) * cw, cy = ol.arena[2] + ((float)iy + 0.5f) * ch;
    const size_t chan = (size_t)gh * gw;
    float *out = d_out + ((size_t)e * C + ch0) * chan + cell;
    for (int m = 0; m < M; ++m) {
        float best, brx, bry;
        out[m * chan] = kb_object_walk(I, m, I.frame[m], cx, cy, best, brx, bry) ? 1.0f : 0.0f;
    }
}

// ---- kb_render: RGB frames of every env ------------------------------------------------------------------------------------
#ifndef KB_RENDER_SINCOS
#define KB_RENDER_SINCOS 1              // sine and cosine of the winning kilobot: 1 once per kilobot into LDS before the walk, 0 per covered pixel (A/B knob)
#endif
constexpr int RENDER_LDS_LIMIT = 64 * 1024;     // the default limit for dynamic LDS: no attribute to raise
constexpr int RENDER_BAND_PIXELS = 8192;        // at most 32 pixels per lane and band: a large frame of a single env still fills the chip
struct RenderArgs {         // the host constants of the definition (include/kilobots_hip.h) and the style, colours as 0x00RRGGBB
    int width, height, layers, bands, band_rows, nlights;
    float cw, ch, Ro2, Ri, Ri2, Lf, Hw, Rl2[KB_MAX_LIGHTS];
    unsigned table, body, ring, mark, light, alpha, obj[KB_MAX_OBJECTS];
};
struct RenderLds {      // byte offsets: the ObjectsLds image at 0, ocol[8] (u32), lit[4] (float4: x, y, Rl2), lcol (uint4: the light's share of the blend and 255 - alpha) --
                        // constants, which cost no register --, then pos (float2), sc (float2: sin, cos), nextb, cellOf, head (u16 each), stage (bytes)
    static constexpr int ocol = ObjectsLds().bytes, lit = ocol + 4 * KB_MAX_OBJECTS, lcol = lit + 16 * KB_MAX_LIGHTS, pos = lcol + 16;
    int sc, nextb, cellOf, head, stage, bands, rows, bytes;
    // the rows of a band: what fits behind the fixed part (3 width bytes each; up to 15 bytes of misalignment of the band in
    // d_rgb in front and the rounding to 16 behind), at most RENDER_BAND_PIXELS pixels, at least one; then the fewest such
    // bands, rows spread evenly over them
    static constexpr int max_rows(int room, int width) {
        const int fit = (room - 32) / (3 * width), cap = RENDER_BAND_PIXELS / width;
        return fit < cap ? (fit > 1 ? fit : 1) : (cap > 1 ? cap : 1);
    }
    __host__ __device__ constexpr RenderLds(int NP, int ncell, int width, int height)
        : sc(pos + 8 * NP), nextb(sc + (KB_RENDER_SINCOS ? 8 * NP : 0)), cellOf(nextb + 2 * NP), head(cellOf + 2 * NP),
          stage((head + 2 * ((ncell + 1) & ~1) + 15) & ~15),
          bands((height + max_rows(RENDER_LDS_LIMIT - stage, width) - 1) / max_rows(RENDER_LDS_LIMIT - stage, width)),
          rows((height + bands - 1) / bands), bytes(stage + ((3 * rows * width + 15 + 15) & ~15)) {}
};
static_assert(ObjectsLds().bytes % 16 == 0, "kb_render_kernel: lit, lcol and pos start on 16 bytes");
static_assert(RenderLds(KB_MAX_BOTS, MAX_CELLS, KB_RENDER_MAX_SIDE, KB_RENDER_MAX_SIDE).bytes <= RENDER_LDS_LIMIT &&
              RenderLds(KB_MAX_BOTS, MAX_CELLS, 64, 48).bands == 1, "kb_render_kernel: LDS image");

// RGB frames (kb_render): one workgroup per (env, band of rows), one pixel per lane and pass.  GATHER: the workgroup builds the
// env's cell lists (kb_build_cell_lists) and every pixel walks the cells within reach of its own (kb_walk_in_range with a = -1:
// no kilobot is excluded), its cell computed from (px, py) as a kilobot's is.  It keeps the highest index among the hits with
// dd <= Ro2 -- the walk lets a NaN through -- so nothing depends on the order of the chains and no pixel is ever updated by
// two lanes.  The walk finds every covering kilobot, those outside the arena too: the cell index along an axis is
// clamp(floor(fl(fl(v - min) * inv_cell))), monotone in v, and two coordinates within Ro of each other give unclamped indices
// at most sense_reach(Ro, inv_cell) apart (the argument of sense_reach); the clamp to the grid maps both monotonically and moves
// no two indices further apart, and a pixel centre's own index is clamped like any other.
// Then the winner's frame (sine and cosine from LDS, one kb_sincosf per kilobot ahead of the walk, or per covered pixel:
// KB_RENDER_SINCOS), the objects for pixels no kilobot covers (kb_stage_objects + kb_object_walk, as kb_grid_objects_kernel;
// every lane of a wave asks about the same object m, so the walk's scalar loop bounds hold), the light discs, and three bytes
// into the band's staging area in LDS: 64 lanes write 192 consecutive bytes, at most two lanes to a word, which costs a store
// nothing.  After one barrier the band leaves as 16-byte stores: its bytes are staged at the offset `mis` that
// its first byte has from a 16-byte boundary of d_rgb, so that every aligned chunk of LDS is an aligned chunk of memory,
// whatever the width; the (at most two) chunks the band only partly owns are written byte by byte.
__global__ void __launch_bounds__(256) kb_render_kernel(const Params p, const kb_outline ol, const RenderArgs A, const int s,
                                                        const unsigned *body_rgb, const unsigned *mark_rgb, unsigned char *d_rgb) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, nt = blockDim.x, N = p.N, W = A.width, H = A.height;
    const int e = blockIdx.x / A.bands, row0 = (blockIdx.x % A.bands) * A.band_rows, rows = min(A.band_rows, H - row0);
    const RenderLds L(p.NP, p.ncell, W, H);
    const ObjectsImage I(smem);
    unsigned *ocol = reinterpret_cast<unsigned *>(smem + L.ocol);
    float4 *lit = reinterpret_cast<float4 *>(smem + L.lit);
    uint4 *lcol = reinterpret_cast<uint4 *>(smem + L.lcol);
    float2 *pos = reinterpret_cast<float2 *>(smem + L.pos);
    float2 *sc = reinterpret_cast<float2 *>(smem + L.sc);
    unsigned short *nextb = reinterpret_cast<unsigned short *>(smem + L.nextb);
    unsigned short *cellOf = reinterpret_cast<unsigned short *>(smem + L.cellOf);
    unsigned short *head = reinterpret_cast<unsigned short *>(smem + L.head);
    unsigned char *stage = smem + L.stage;
    const size_t o = (size_t)e * N;
    const bool bots = (A.layers & KB_RENDER_BOTS) != 0;
    const int M = (A.layers & KB_RENDER_OBJECTS) ? ol.num_objects : 0, nlights = A.nlights;
    // the tables a pixel indexes by a run-time number go through LDS (they arrive in scalar registers, which cannot be indexed)
#pragma unroll
    for (int m = 0; m < KB_MAX_OBJECTS; ++m) if (tid == 64 + m) ocol[m] = A.obj[m];
#pragma unroll
    for (int l = 0; l < KB_MAX_LIGHTS; ++l) {
        if (tid == 96 + l && l < nlights)
            lit[l] = make_float4(p.buf.light_x[(size_t)e * nlights + l] * WORLD_SCALE, p.buf.light_y[(size_t)e * nlights + l] * WORLD_SCALE, A.Rl2[l], 0.0f);
    }
    if (tid == 100) lcol[0] = make_uint4(((A.light >> 16) & 255u) * A.alpha + 127u, ((A.light >> 8) & 255u) * A.alpha + 127u, (A.light & 255u) * A.alpha + 127u, 255u - A.alpha);
    if (M > 0) kb_stage_objects(ol, I, e, tid, p.buf.ox, p.buf.oy, p.buf.otheta);
    if (bots) {
        if (KB_RENDER_SINCOS) {
            for (int b = tid; b < N; b += nt) {
                float sn, cs;
                kb_sincosf(p.buf.theta[o + b], sn, cs);
                sc[b] = make_float2(sn, cs);
            }
        }
        kb_build_cell_lists(p, o, pos, head, nextb, cellOf, tid, nt);
    } else {
        __syncthreads();
    }
    // (the low bits of the address of the band's first byte: 32-bit arithmetic, which may wrap, gives them)
    const int mis = (int)(((unsigned)reinterpret_cast<uintptr_t>(d_rgb) + ((unsigned)e * (unsigned)H + (unsigned)row0) * (unsigned)W * 3u) & 15u);
    const int npix = rows * W;
    const int q256 = nt / W, r256 = nt % W;
    int r = tid / W, i = tid % W;
    for (int f = tid; f < npix; f += nt) {
        const float px = p.xmin + ((float)i + 0.5f) * A.cw;
        const float py = p.ymin + ((float)(H - 1 - (row0 + r)) + 0.5f) * A.ch;
        unsigned col = A.table;
        int win = -1;
        if (bots) {
            int cx = (int)floorf((px - p.xmin) * p.inv_cell);
            int cy = (int)floorf((py - p.ymin) * p.inv_cell);
            cx = cx < 0 ? 0 : (cx >= p.gw ? p.gw - 1 : cx);
            cy = cy < 0 ? 0 : (cy >= p.gh ? p.gh - 1 : cy);
            kb_walk_in_range(p, pos, head, nextb, -1, cy * p.gw + cx, make_float2(px, py), s, A.Ro2, [&](unsigned b, float, float, float dd) {
                if (dd <= A.Ro2) win = max(win, (int)b);
            });
        }
        if (win >= 0) {
            const float2 pb = pos[win];
            const float qx = px - pb.x, qy = py - pb.y;
            const float dd = qx * qx + qy * qy;
            float sn, cs;
            if (KB_RENDER_SINCOS) { const float2 t = sc[win]; sn = t.x; cs = t.y; }
            else kb_sincosf(p.buf.theta[o + win], sn, cs);
            const float a = cs * qx + sn * qy, l = cs * qy - sn * qx;
            if (A.Lf > 0.0f && a >= 0.0f && a <= A.Lf && fabsf(l) <= A.Hw) col = mark_rgb ? mark_rgb[o + win] : A.mark;
            else if (!(A.Ri > 0.0f) || dd > A.Ri2) col = A.ring;
            else col = body_rgb ? body_rgb[o + win] : A.body;
        } else {
            for (int m = 0; m < M; ++m) {
                float best, brx, bry;
                if (kb_object_walk(I, m, I.frame[m], px, py, best, brx, bry)) col = ocol[m];
            }
        }
        unsigned cr = (col >> 16) & 255u, cg = (col >> 8) & 255u, cb = col & 255u;
        for (int l = 0; l < nlights; ++l) {
            const float4 lt = lit[l];
            const float fx = lt.x - px, fy = lt.y - py;
            if (fx * fx + fy * fy <= lt.z) {
                const uint4 lc = lcol[0];       // (light_c * A + 127 per channel, 255 - A)
                cr = (lc.x + cr * lc.w) / 255u;
                cg = (lc.y + cg * lc.w) / 255u;
                cb = (lc.z + cb * lc.w) / 255u;
            }
        }
        unsigned char *dst = stage + mis + 3 * f;
        dst[0] = (unsigned char)cr; dst[1] = (unsigned char)cg; dst[2] = (unsigned char)cb;
        r += q256; i += r256;
        if (i >= W) { i -= W; r++; }
    }
    __syncthreads();
    const int end = mis + 3 * npix;         // the band's bytes are stage[mis .. end)
    const size_t first = ((size_t)e * H + row0) * (size_t)W * 3;        // the band's first byte in d_rgb
    unsigned char *base = d_rgb + first - mis;      // 16-byte aligned; nothing before base + mis or from base + end on is touched
    for (int c = tid; 16 * c < end; c += nt) {
        const int lo = 16 * c;
        if (lo >= mis && lo + 16 <= end) {
            reinterpret_cast<uint4 *>(base)[c] = reinterpret_cast<const uint4 *>(stage)[c];
        } else {
            for (int k = max(lo, mis); k < min(lo + 16, end); ++k) base[k] = stage[k];
        }
    }
}

// ---- kb_sense_rays: first-hit range scans in every kilobot's frame -----------------------------------------------------------
struct RayArgs {            // the host constants of the definition (include/kilobots_hip.h) and the direction table of kb_ray_directions
    int n_rays, targets;
    float Rw, Rc2, rb2;
    float ux[KB_MAX_RAYS], uy[KB_MAX_RAYS];     // (0, 0) behind n_rays: such a ray is computed like any other and never stored
};
struct RaysLds {        // byte offsets: pos (float2) at 0, nextb, cellOf, head (u16 each), dir[32] (float2), vert[F][4] (float2: world frame), wall[4][2] (float2), fix[F] (float4)
    int nextb, cellOf, head, dir, vert, wall, fix, bytes;
    __host__ __device__ constexpr RaysLds(int NP, int ncell)
        : nextb(8 * NP), cellOf(10 * NP), head(12 * NP), dir((head + 2 * ((ncell + 1) & ~1) + 15) & ~15),
          vert(dir + 8 * KB_MAX_RAYS), wall(vert + 8 * OBJ_EDGES), fix(wall + 8 * 8), bytes(fix + 16 * KB_MAX_OBJECTS) {}
};
// the largest image (1024 kilobots, every cell) stays under the default limit for dynamic LDS: no attribute to raise
static_assert(RaysLds(KB_MAX_BOTS, MAX_CELLS).bytes <= 64 * 1024, "kb_rays_kernel: LDS image");

// The world vector (dx, dy) from a kilobot with heading (sn, cs) along and across each of the R rays of u: b[k], q[k].
template <int R>
__device__ __forceinline__ void kb_ray_project(const float2 *u, const float sn, const float cs, const float dx, const float dy,
                                               float *b, float *q) {
    const float a = cs * dx + sn * dy, l = cs * dy - sn * dx;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const float2 d = u[k];      // (the same address in every lane: a broadcast)
        b[k] = a * d.x + l * d.y;
        q[k] = a * d.y - l * d.x;
    }
}

// The best key of one ray against candidate `code` at parameter t: (bits(t + 0) << 32) | code, compared unsigned.  The key
// starts as (bits(Rw) << 32) | 0xFFFFFFFF, so whatever undercuts it has +0 <= t <= Rw: a negative t and a NaN (a miss of the
// formulas above it) have larger bits than any Rw, "t <= Rw" and "nothing hit" need no flag, and t + 0 is t except that it
// turns -0 into the +0 the definition asks for.  One comparison per ray and candidate: with a flag per rule of the
// definition the 16-ray code held more lane masks than there are scalar registers.
__device__ __forceinline__ void kb_ray_take(unsigned long long &best, const unsigned tbits, const unsigned code) {
    const unsigned long long key = ((unsigned long long)tbits << 32) | code;
    best = key < best ? key : best;
}

// A disc of squared radius r2 whose centre projects to (b, q), ray by ray.  h2 < 0 makes sq, t1, t2 and t NaN; t2 < 0 makes
// t = t2 negative: both miss.
template <int R>
__device__ __forceinline__ void kb_ray_disc(const float *b, const float *q, const float r2, const unsigned code, unsigned long long *best) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const float h2 = r2 - q[k] * q[k];
        const float sq = sqrtf(h2);
        const float t1 = b[k] - sq, t2 = b[k] + sq;
        const float t = t1 >= 0.0f ? t1 : t2;
        kb_ray_take(best[k], __float_as_uint(t + 0.0f), code);
    }
}

// The segment from the vertex that projects to (bA, qA) to the one that projects to (bB, qB), ray by ray.  It straddles the
// ray iff min(qA, qB) <= 0 <= max(qA, qB), i.e. iff w = max(min(qA, qB), min(-qA, -qB)) <= 0; a straddling segment with
// den == 0 has qA = qB = 0, sg = 0 / 0 and t NaN, and a NaN among the q makes t NaN: both miss.
template <int R>
__device__ __forceinline__ void kb_ray_segment(const float *bA, const float *qA, const float *bB, const float *qB, const unsigned code,
                                               unsigned long long *best) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const float w = fmaxf(fminf(qA[k], qB[k]), fminf(-qA[k], -qB[k]));
        const float den = qA[k] - qB[k];
        const float sg = qA[k] / den;
        const float t = bA[k] + sg * (bB[k] - bA[k]);
        kb_ray_take(best[k], w <= 0.0f ? __float_as_uint(t + 0.0f) : 0xFFFFFFFFu, code);
    }
}

// The fixtures and the walls of the staged env against G rays of one kilobot at (xi, yi) with heading (sn, cs): fixtures ->
// vertices with (b, q) of the previous vertex carried in registers, so that a vertex is projected once per ray for both its
// edges (vertex 0 a second time, to close the outline: the same operations, the same bits); the NW walls, a segment each.
// All table reads are from LDS at addresses that are the same in every lane (broadcasts); the loop bounds are the same in
// all lanes and are made scalar with readfirstlane, as in kb_object_walk.  The loops over the edges and the walls are kept
// rolled and the kernel calls this for four rays at a time: the G correctly rounded divisions of an edge are scheduled
// side by side, and with 16 rays, or with the walls unrolled, that took all 256 VGPRs.
template <int G>
__device__ __forceinline__ void kb_ray_outlines(const float2 *u, const float sn, const float cs, const float xi, const float yi, const float2 *vert,
                                                const float2 *wall, const float4 *fix, const int F, const int NW, const int N, unsigned long long *best) {
    for (int f = 0; f < F; ++f) {
        const float4 fx = fix[f];
        const int n = __builtin_amdgcn_readfirstlane(__float_as_int(fx.x));
        const unsigned code = (unsigned)__builtin_amdgcn_readfirstlane(__float_as_int(fx.y));
        const float2 v0 = vert[KB_MAX_POLY_VERTS * f];
        float bp[G], qp[G];
        kb_ray_project<G>(u, sn, cs, v0.x - xi, v0.y - yi, bp, qp);
        if (n == 0) {
            kb_ray_disc<G>(bp, qp, fx.z, code, best);
        } else {
#pragma unroll 1
            for (int k = 1; k <= n; ++k) {
                const float2 v = vert[KB_MAX_POLY_VERTS * f + (k == n ? 0 : k)];
                float bc[G], qc[G];
                kb_ray_project<G>(u, sn, cs, v.x - xi, v.y - yi, bc, qc);
                kb_ray_segment<G>(bp, qp, bc, qc, code, best);
#pragma unroll
                for (int i = 0; i < G; ++i) { bp[i] = bc[i]; qp[i] = qc[i]; }
            }
        }
    }
#pragma unroll 1
    for (int w = 0; w < NW; ++w) {
        const float2 va = wall[2 * w], vb = wall[2 * w + 1];
        float bA[G], qA[G], bB[G], qB[G];
        kb_ray_project<G>(u, sn, cs, va.x - xi, va.y - yi, bA, qA);
        kb_ray_project<G>(u, sn, cs, vb.x - xi, vb.y - yi, bB, qB);
        kb_ray_segment<G>(bA, qA, bB, qB, (unsigned)(N + w), best);
    }
}

constexpr int RAY_GROUP = 4;
#ifndef KB_RAYS_PER_PASS
#define KB_RAYS_PER_PASS 16             // the most rays kb_rays_kernel keeps in registers at a time: 8 or 16 (A/B knob)
#endif
static_assert(KB_RAYS_PER_PASS == 8 || KB_RAYS_PER_PASS == 16, "kb_rays_kernel: rays per pass");

// Range scans on the current poses (kb_sense_rays): one workgroup per env, one kilobot per lane, like kb_neighbors_kernel.
// Poses and the cell lists in LDS (kb_build_cell_lists); a kilobot's own pose and heading are used by its own lane only and are
// read straight from global memory into registers, as in kb_histogram_kernel.  Once per workgroup the direction table, the
// env's fixture vertices in the WORLD frame (lane 64 + 4 f + k rotates vertex k of fixture f by its body's frame; a circle's
// centre takes the place of vertex 0), per fixture (vertex count, code N + 4 + body, r * r) and the two ends of every wall go
// to LDS -- values every lane would otherwise compute for itself, each a single fp32 operation and therefore the same bits
// whoever evaluates it.  A lane then reads them at addresses that are the same in every lane (broadcasts).
// Candidates: the kilobots through kb_walk_in_range at the reach of Rc = Rw + r_bot, then the fixtures and the walls, four
// rays at a time (kb_ray_outlines).
// The best key of every ray stays in registers: RP rays are processed at a time -- the ray count rounded up to 4, 8 or 16,
// and 17 to 32 rays in two passes of 16 over the candidates (KB_RAYS_PER_PASS) -- and every index into best[], b[] and q[] is
// a compile-time constant.  The winner of a ray does not depend on the order of the candidates, and no ray on another ray:
// the passes give what one pass would.  Rays behind n_rays have the direction (0, 0), are computed and never stored.
// Each lane stores its own rows: 16 bytes per store with vec (n_rays a multiple of 4, d_dist and d_hit 16-byte aligned).
template <int RP>
__global__ void __launch_bounds__(256) kb_rays_kernel(const Params p, const kb_outline ol, const RayArgs A, const int s, const int vec,
                                                      float *d_dist, int *d_hit) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, N = p.N, n_rays = A.n_rays;
    const RaysLds L(p.NP, p.ncell);
    float2 *pos = reinterpret_cast<float2 *>(smem);
    unsigned short *nextb = reinterpret_cast<unsigned short *>(smem + L.nextb);
    unsigned short *cellOf = reinterpret_cast<unsigned short *>(smem + L.cellOf);
    unsigned short *head = reinterpret_cast<unsigned short *>(smem + L.head);
    float2 *dir = reinterpret_cast<float2 *>(smem + L.dir);
    float2 *vert = reinterpret_cast<float2 *>(smem + L.vert);
    float2 *wall = reinterpret_cast<float2 *>(smem + L.wall);
    float4 *fix = reinterpret_cast<float4 *>(smem + L.fix);
    const size_t o = (size_t)e * N;
    const bool bots = (A.targets & KB_RAY_BOTS) != 0;
    const int F = (A.targets & KB_RAY_OBJECTS) ? ol.num_fixtures : 0, NW = (A.targets & KB_RAY_WALLS) ? 4 : 0;
    if (tid < KB_MAX_RAYS) dir[tid] = make_float2(A.ux[tid], A.uy[tid]);
    if (tid >= 64 && tid < 64 + OBJ_EDGES) {
        const int f = (tid - 64) / KB_MAX_POLY_VERTS, k = (tid - 64) % KB_MAX_POLY_VERTS;
        if (f < F) {
            const int n = ol.nverts[f], m = ol.body[f];
            const size_t j = (size_t)e * ol.num_objects + m;
            const float ox = p.buf.ox[j], oy = p.buf.oy[j];
            float so, co;
            kb_sincosf(p.buf.otheta[j], so, co);
            const float vx = ol.verts[f][k][0], vy = ol.verts[f][k][1];
            if (k < n) vert[tid - 64] = make_float2(ox + (co * vx - so * vy), oy + (so * vx + co * vy));
            if (k == 0) {
                if (n == 0) vert[tid - 64] = make_float2(ox, oy);
                const float r = ol.radius[f];
                fix[f] = make_float4(__int_as_float(n), __int_as_float(N + 4 + m), r * r, 0.0f);
            }
        }
    }
    if (tid >= 128 && tid < 136) {      // wall w from wall[2 w] to wall[2 w + 1]: W0, W1 run up the xmin and the xmax side, W2, W3 along ymin and ymax
        const int w = (tid - 128) >> 1, far = (tid - 128) & 1;
        wall[tid - 128] = make_float2(w == 1 || (w >= 2 && far) ? ol.arena[1] : ol.arena[0], (w < 2 ? far : w == 3) ? ol.arena[3] : ol.arena[2]);
    }
    if (bots) kb_build_cell_lists(p, o, pos, head, nextb, cellOf, tid, nt);
    else __syncthreads();
    for (int a = tid; a < N; a += nt) {
        const float xi = p.buf.x[o + a], yi = p.buf.y[o + a];
        float sn, cs;
        kb_sincosf(p.buf.theta[o + a], sn, cs);
        const size_t row = (o + a) * (size_t)n_rays;
        for (int k0 = 0; k0 < n_rays; k0 += RP) {
            const float2 *u = dir + k0;
            unsigned long long best[RP];
#pragma unroll
            for (int k = 0; k < RP; ++k) best[k] = ((unsigned long long)__float_as_uint(A.Rw) << 32) | 0xFFFFFFFFull;
            if (bots) {
                kb_walk_in_range(p, pos, head, nextb, a, (int)cellOf[a], make_float2(xi, yi), s, A.Rc2, [&](unsigned j, float ex, float ey, float) {
                    float b[RP], q[RP];
                    kb_ray_project<RP>(u, sn, cs, ex, ey, b, q);
                    kb_ray_disc<RP>(b, q, A.rb2, j, best);
                });
            }
#pragma unroll
            for (int g = 0; g < RP; g += RAY_GROUP) kb_ray_outlines<RAY_GROUP>(u + g, sn, cs, xi, yi, vert, wall, fix, F, NW, N, best + g);
            float *dist = d_dist + row + k0;
            int *hit = d_hit ? d_hit + row + k0 : nullptr;
            if (vec) {
#pragma unroll
                for (int i = 0; i < RP; i += 4) {
                    if (k0 + i >= n_rays) continue;
                    reinterpret_cast<float4 *>(dist)[i >> 2] = make_float4(__uint_as_float((unsigned)(best[i] >> 32)) / WORLD_SCALE, __uint_as_float((unsigned)(best[i + 1] >> 32)) / WORLD_SCALE,
                                                                           __uint_as_float((unsigned)(best[i + 2] >> 32)) / WORLD_SCALE, __uint_as_float((unsigned)(best[i + 3] >> 32)) / WORLD_SCALE);
                    if (hit) reinterpret_cast<int4 *>(hit)[i >> 2] = make_int4((int)(unsigned)best[i], (int)(unsigned)best[i + 1], (int)(unsigned)best[i + 2], (int)(unsigned)best[i + 3]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < RP; ++i) {
                    if (k0 + i >= n_rays) continue;
                    dist[i] = __uint_as_float((unsigned)(best[i] >> 32)) / WORLD_SCALE;
                    if (hit) hit[i] = (int)(unsigned)best[i];       // (the low word of a ray that hit nothing is -1)
                }
            }
        }
    }
}

// ---- kb_sense_edges: the whole IR-range graph as a CSR edge list --------------------------------------------------------------
constexpr int EDGE_TILE = 256;          // rows (= lanes) per tile of kb_edges_kernel
struct EdgesLds {       // byte offsets: pos (float2) at 0, th (float), nextb, head (u16 each), mask[EDGE_TILE][stride] (u32); cellOf (u16) lies over mask
    int th, nextb, head, mask, words, stride, bytes;
    // words: of a row's bitmask, one bit per kilobot of the env; stride: the next odd number, so that word w of the rows of
    // consecutive lanes lies in consecutive banks.  cellOf is read once, before the first mask is cleared, and needs no room of its own.
    __host__ __device__ constexpr EdgesLds(int N, int NP, int ncell)
        : th(8 * NP), nextb(12 * NP), head(14 * NP), mask(head + 2 * ((ncell + 1) & ~1)), words((N + 31) >> 5), stride(words | 1),
          bytes(mask + (4 * EDGE_TILE * stride > 2 * NP ? 4 * EDGE_TILE * stride : 2 * NP)) {}
};
// the largest image (1024 kilobots, every cell) stays under the default limit for dynamic LDS: no attribute to raise
static_assert(EdgesLds(KB_MAX_BOTS, KB_MAX_BOTS, MAX_CELLS).bytes <= 64 * 1024, "kb_edges_kernel: LDS image");
static_assert(KB_MAX_BOTS <= 4 * EDGE_TILE, "kb_edges_kernel: a lane keeps the cells of at most four rows");

// The IR-range graph on the current poses (kb_sense_edges): every pair of kilobots in range, both directions, as rows of a
// CSR list whose row pointer the caller supplies.  Poses, headings and the cell lists in LDS, one kilobot (= row) per lane
// over the full stencil, like kb_neighbors_kernel, in tiles of EDGE_TILE rows.  The chains of the cell lists are in exchange
// order, so the order of a row is MADE: the lane owns a bitmask of one bit per kilobot of the env in LDS, clears it, sets bit
// j for every hit of the walk (plain read-modify-write: nobody else touches the row, no atomics, no barrier inside the tile
// loop) and then scans the words upwards, lowest set bit first -- ascending j by construction, whatever the walk's order.
// An edge's attributes are recomputed from pos[j] and th[j] with the operations of kb_neighbors_kernel (d2 is the walk's dd:
// the same operations on the same operands, the same bits).
// Memory contract: row r owns the slots [lo, hi) of d_offsets[r], d_offsets[r + 1], both clipped to [0, capacity]; the lane
// writes the first min(count, hi - lo) neighbours there and -1 / +0.0 into what is left of the row, and stores nowhere else.
// Emission is per lane: 4 + 4 + 16 bytes per edge at the lane's own cursor.
__global__ void __launch_bounds__(256) kb_edges_kernel(const Params p, const int s, const float R2, const long long *d_offsets, const long long capacity,
                                                       int *d_src, int *d_dst, float4 *d_rel, unsigned *d_count) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, N = p.N;
    const EdgesLds L(N, p.NP, p.ncell);
    float2 *pos = reinterpret_cast<float2 *>(smem);
    float *th = reinterpret_cast<float *>(smem + L.th);
    unsigned short *nextb = reinterpret_cast<unsigned short *>(smem + L.nextb);
    unsigned short *head = reinterpret_cast<unsigned short *>(smem + L.head);
    unsigned short *cellOf = reinterpret_cast<unsigned short *>(smem + L.mask);
    unsigned *row = reinterpret_cast<unsigned *>(smem + L.mask) + tid * L.stride;
    const size_t o = (size_t)e * N;
    for (int b = tid; b < N; b += nt) th[b] = p.buf.theta[o + b];
    kb_build_cell_lists(p, o, pos, head, nextb, cellOf, tid, nt);
    // the cells of the lane's (at most four) rows, two to a register, before the masks take cellOf's place
    unsigned c01 = 0, c23 = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int a = tid + t * EDGE_TILE;
        const unsigned c = a < N ? (unsigned)cellOf[a] : 0u;
        if (t < 2) c01 |= c << (16 * t);
        else c23 |= c << (16 * (t - 2));
    }
    __syncthreads();
    const int W = L.words;
    for (int t = 0; t * EDGE_TILE < N; ++t) {
        const int a = t * EDGE_TILE + tid;
        if (a >= N) break;      // (no barrier follows)
        const int cell = (int)(((t < 2 ? c01 : c23) >> (16 * (t & 1))) & 0xFFFFu);
        const float2 pa = pos[a];
        for (int w = 0; w < W; ++w) row[w] = 0u;
        const unsigned cnt = kb_walk_in_range(p, pos, head, nextb, a, cell, pa, s, R2, [&](unsigned b, float, float, float) {
            row[b >> 5] |= 1u << (b & 31u);
        });
        if (d_count) d_count[o + a] = cnt;
        if (capacity <= 0) continue;
        const long long o0 = d_offsets[o + a], o1 = d_offsets[o + a + 1];
        const long long lo = o0 < 0 ? 0 : (o0 > capacity ? capacity : o0), hi = o1 < 0 ? 0 : (o1 > capacity ? capacity : o1);
        if (hi <= lo) continue;
        const float tha = th[a];
        float sn, cs;
        kb_sincosf(tha, sn, cs);
        const int node0 = (int)o, src = node0 + a;
        long long slot = lo;
        for (int w = 0; w < W && slot < hi; ++w) {
            for (unsigned bits = row[w]; bits != 0u && slot < hi; bits &= bits - 1u, ++slot) {
                const int j = 32 * w + __builtin_ctz(bits);
                const float2 pb = pos[j];
                const float ex = pb.x - pa.x, ey = pb.y - pa.y;
                const float d2 = ex * ex + ey * ey;
                d_dst[slot] = node0 + j;
                if (d_src) d_src[slot] = src;
                if (d_rel) d_rel[slot] = make_float4((cs * ex + sn * ey) / WORLD_SCALE, (cs * ey - sn * ex) / WORLD_SCALE, sqrtf(d2) / WORLD_SCALE, th[j] - tha);
            }
        }
        for (; slot < hi; ++slot) {     // offsets that give the row more than it has
            d_dst[slot] = -1;
            if (d_src) d_src[slot] = -1;
            if (d_rel) d_rel[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

// ---- kb_sense_contacts: touch and push sensing from the warm-start store ---------------------------------------------------
constexpr unsigned WS_WALL = 0x10000u, WS_OBJ = 0x20000u;      // the key classes the step writes into ws_key
struct ContactsArgs {       // the handle's fixture -> body table (kb_config numbering) and what the kernel needs of Params
    int N, M, F, cap;
    int body[KB_MAX_OBJECTS];
};
struct ContactsLds {        // byte offsets of u32 arrays: off[NP4 + 1] at 0, ioff[NP4 + 1], icnt[NP4], qin[NP4], own[NP4], oacc[2 M], fb[F], wsum[4]
    int NP4, ioff, icnt, qin, own, oacc, fb, wsum, bytes;
    __host__ __device__ constexpr ContactsLds(int N)
        : NP4((N + 3) & ~3), ioff(4 * (NP4 + 4)), icnt(2 * ioff), qin(icnt + 4 * NP4), own(qin + 4 * NP4), oacc(own + 4 * NP4),
          fb(oacc + 8 * KB_MAX_OBJECTS), wsum(fb + 4 * KB_MAX_OBJECTS), bytes(wsum + 16) {}
};
static_assert(ContactsLds(KB_MAX_BOTS).bytes <= 64 * 1024, "kb_contacts_kernel: LDS image");

// Exclusive scan in place of the NP4 (a multiple of 4, <= 4 * blockDim.x) u32 words of v, which start on 16 bytes; v[NP4]
// receives the total.  All threads must call; two workgroup barriers inside, the second behind the last store.
__device__ __forceinline__ void kb_block_scan_u32(unsigned *v, const int NP4, unsigned *wsum, const int tid) {
    const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const bool in = 4 * tid < NP4;
    const uint4 c = in ? reinterpret_cast<const uint4 *>(v)[tid] : make_uint4(0u, 0u, 0u, 0u);
    const unsigned sum = c.x + c.y + c.z + c.w;
    const unsigned incl = wave_incl_scan(sum);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned base = incl - sum;
    for (int w = 0; w < nw; ++w) { const unsigned s = wsum[w]; if (w < wave) base += s; }
    if (in) {
        uint4 r;
        r.x = base; r.y = r.x + c.x; r.z = r.y + c.y; r.w = r.z + c.z;
        reinterpret_cast<uint4 *>(v)[tid] = r;
        if (4 * tid + 4 == NP4) v[NP4] = r.w + c.w;
    }
    __syncthreads();
}

// What entry `key` of kilobot a is: 0 nothing (a key of no class, the kilobot itself), 1 a kilobot, 2 a wall, 3 a fixture;
// code: the public partner code (kilobot; N + wall in the order of kb_sense_objects; N + 4 + object), sub: the fixture.
__device__ __forceinline__ int kb_contact_class(const unsigned key, const int a, const int N, const int F, const unsigned *fb,
                                                unsigned &code, unsigned &sub) {
    sub = 0u;
    if (key < (unsigned)N) { code = key; return key != (unsigned)a ? 1 : 0; }
    const unsigned w = key - WS_WALL;
    if (w < 4u) { code = (unsigned)N + ((w & 1u) << 1 | w >> 1); return 2; }      // store: xmin ymin xmax ymax; public: xmin xmax ymin ymax
    const unsigned f = key - WS_OBJ;
    if (key >= WS_OBJ && f < (unsigned)F) { code = (unsigned)N + 4u + fb[f]; sub = f; return 3; }
    code = 0u;
    return 0;
}

// Touch and push sensing from the contact store of the last step (kb_sense_contacts): one workgroup per env, one kilobot per
// lane and pass.  The store lists a kilobot-kilobot contact under one of its two kilobots only; every kilobot reports it.
//   1. ws_cnt -> off (u32: a store past its capacity may count more than 65535 entries), exclusive scan (kb_block_scan_u32).
//   2. Owner pass: every kilobot walks its own entries (those behind the capacity were never stored).  Wall and fixture
//      entries count in its registers; a kilobot entry counts there and adds 1 to icnt[partner] and the fixed-point image of
//      its impulse (kb_reduce_quant) to qin[partner] with LDS atomics whose result is not used -- integer adds, so the sums
//      do not depend on the order.  Fixture entries add likewise to the 2 M words of the object rows.
//   3. K > 0: icnt -> ioff, scan, and every owner hands each kilobot entry to its partner as (owner, impulse bits), 8 bytes,
//      at ioff[partner] + a cursor (icnt, counted down) in the env's slice of kb_buffers.scratch: at most one record per
//      stored entry, cap * 8 of the slice's cap * 32 bytes.  The records change hands through global memory: __syncthreads().
//   4. Gather: every kilobot runs its own and its incoming entries down the compare-exchange chain of kb_neighbors_kernel on
//      ((code * 8 + fixture) << 32) | impulse bits -- best[] is indexed by constants only and stays in registers -- so
//      neither the order of the store nor that of the cursors shows.  Rows go out per lane, 16 bytes per store with vec.
// K: the requested k rounded up to 4, 8 or 16; 0: no lists (steps 3 and the chain are not compiled).
template <int K>
__global__ void __launch_bounds__(256) kb_contacts_kernel(const ContactsArgs A, const int k, const int vec, const float scale, const unsigned *ws_key,
                                                          const float *ws_acc, const unsigned char *ws_cnt, uint2 *slice, int *d_partner,
                                                          float *d_impulse, float *d_touch, float *d_obj) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr unsigned long long NONE = ~0ull;
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, N = A.N, M = A.M, F = A.F, cap = A.cap;
    const ContactsLds L(N);
    unsigned *off = reinterpret_cast<unsigned *>(smem);
    unsigned *ioff = reinterpret_cast<unsigned *>(smem + L.ioff);
    unsigned *icnt = reinterpret_cast<unsigned *>(smem + L.icnt);
    unsigned *qin = reinterpret_cast<unsigned *>(smem + L.qin);
    unsigned *own = reinterpret_cast<unsigned *>(smem + L.own);
    unsigned *oacc = reinterpret_cast<unsigned *>(smem + L.oacc);
    unsigned *fb = reinterpret_cast<unsigned *>(smem + L.fb);
    unsigned *wsum = reinterpret_cast<unsigned *>(smem + L.wsum);
    const size_t o = (size_t)e * N;
    const unsigned *wk = ws_key + (size_t)e * cap;
    const float *wa = ws_acc + (size_t)e * cap;
    uint2 *tr = slice + (size_t)e * cap * 4;        // (the env's slice: 32 bytes per contact of the capacity)
    for (int b = tid; b < L.NP4; b += nt) {
        off[b] = b < N ? (unsigned)ws_cnt[o + b] : 0u;
        icnt[b] = 0u; qin[b] = 0u;
    }
    if (tid < 2 * KB_MAX_OBJECTS) oacc[tid] = 0u;
#pragma unroll
    for (int f = 0; f < KB_MAX_OBJECTS; ++f) if (tid == f) fb[f] = (unsigned)A.body[f];
    __syncthreads();
    kb_block_scan_u32(off, L.NP4, wsum, tid);
    for (int a = tid; a < N; a += nt) {
        const unsigned p1 = min(off[a + 1], (unsigned)cap);
        unsigned nk = 0, nw = 0, no = 0, q = 0;
        for (unsigned pos = off[a]; pos < p1; ++pos) {
            const unsigned key = wk[pos];
            const unsigned qi = (unsigned)kb_reduce_quant(wa[pos], scale);
            unsigned code, sub;
            const int cls = kb_contact_class(key, a, N, F, fb, code, sub);
            if (cls) q += qi;
            if (cls == 1) {
                nk++;
                atomicAdd(&icnt[key], 1u);
                atomicAdd(&qin[key], qi);
            } else if (cls == 2) {
                nw++;
            } else if (cls == 3) {
                no++;
                const unsigned m = code - (unsigned)N - 4u;
                atomicAdd(&oacc[2 * m], 1u);
                atomicAdd(&oacc[2 * m + 1], qi);
            }
        }
        own[a] = nk | nw << 10 | no << 20;      // (each at most 255)
        if (q) atomicAdd(&qin[a], q);
    }
    __syncthreads();
    if (d_obj && tid < M) {
        float *row = d_obj + ((size_t)e * M + tid) * 2;
        row[0] = (float)oacc[2 * tid];
        row[1] = (float)(int)oacc[2 * tid + 1] / scale;
    }
    if constexpr (K > 0) {
        for (int b = tid; b < L.NP4; b += nt) ioff[b] = icnt[b];
        __syncthreads();
        kb_block_scan_u32(ioff, L.NP4, wsum, tid);
        for (int a = tid; a < N; a += nt) {
            const unsigned p1 = min(off[a + 1], (unsigned)cap);
            for (unsigned pos = off[a]; pos < p1; ++pos) {
                const unsigned key = wk[pos];
                if (key < (unsigned)N && key != (unsigned)a) {
                    const unsigned slot = ioff[key] + atomicSub(&icnt[key], 1u) - 1u;
                    if (slot < (unsigned)cap) tr[slot] = make_uint2((unsigned)a, __float_as_uint(wa[pos]));
                }
            }
        }
        __syncthreads();        // the records are read by other lanes, from global memory
    }
    for (int a = tid; a < N; a += nt) {
        const unsigned ow = own[a];
        const unsigned i0 = K > 0 ? ioff[a] : 0u, i1 = K > 0 ? min(ioff[a + 1], (unsigned)cap) : 0u;
        if (d_touch) {
            const unsigned nin = K > 0 ? ioff[a + 1] - i0 : icnt[a];
            const float4 t = make_float4((float)((ow & 1023u) + nin), (float)((ow >> 10) & 1023u), (float)(ow >> 20), (float)(int)qin[a] / scale);
            float *row = d_touch + (o + a) * 4;
            if (vec & 2) *reinterpret_cast<float4 *>(row) = t;
            else { row[0] = t.x; row[1] = t.y; row[2] = t.z; row[3] = t.w; }
        }
        if constexpr (K > 0) {
            unsigned long long best[K];
#pragma unroll
            for (int i = 0; i < K; ++i) best[i] = NONE;
            const auto insert = [&](unsigned long long key) {
                if (key < best[K - 1]) {
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        const unsigned long long lo = key < best[j] ? key : best[j];
                        key = key < best[j] ? best[j] : key;
                        best[j] = lo;
                    }
                }
            };
            const unsigned p1 = min(off[a + 1], (unsigned)cap);
            for (unsigned pos = off[a]; pos < p1; ++pos) {
                unsigned code, sub;
                if (kb_contact_class(wk[pos], a, N, F, fb, code, sub))
                    insert(((unsigned long long)(code * 8u + sub) << 32) | __float_as_uint(wa[pos]));
            }
            for (unsigned i = i0; i < i1; ++i) {
                const uint2 r = tr[i];
                insert(((unsigned long long)(r.x * 8u) << 32) | r.y);
            }
            const size_t row = (o + a) * (size_t)k;
            if (vec & 1) {      // k is a multiple of 4, d_partner and d_impulse are 16-byte aligned: four slots per store
#pragma unroll
                for (int i = 0; i < K; i += 4) {
                    if (i >= k) break;
                    int4 c;
                    uint4 b;
                    c.x = best[i] != NONE ? (int)(best[i] >> 35) : -1; b.x = best[i] != NONE ? (unsigned)best[i] : 0u;
                    c.y = best[i + 1] != NONE ? (int)(best[i + 1] >> 35) : -1; b.y = best[i + 1] != NONE ? (unsigned)best[i + 1] : 0u;
                    c.z = best[i + 2] != NONE ? (int)(best[i + 2] >> 35) : -1; b.z = best[i + 2] != NONE ? (unsigned)best[i + 2] : 0u;
                    c.w = best[i + 3] != NONE ? (int)(best[i + 3] >> 35) : -1; b.w = best[i + 3] != NONE ? (unsigned)best[i + 3] : 0u;
                    reinterpret_cast<int4 *>(d_partner + row)[i >> 2] = c;
                    reinterpret_cast<uint4 *>(d_impulse + row)[i >> 2] = b;
                }
            } else {
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    if (i >= k) break;
                    const bool used = best[i] != NONE;
                    d_partner[row + i] = used ? (int)(best[i] >> 35) : -1;
                    reinterpret_cast<unsigned *>(d_impulse)[row + i] = used ? (unsigned)best[i] : 0u;
                }
            }
        }
    }
}

}  // namespace kb
