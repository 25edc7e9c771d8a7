// kb_coopsolve_bins.inc -- cooperative solver of the kernels without objects for envs with a giant island (textually included
// by kb_step_kernel.h inside the substep loop, behind the bucket sort of the contacts by canonical key).
//
// Round 2 swept such an env key by key: ~22 workgroup-wide rounds per pass, 21 passes, every round a walk over bucket list ->
// order -> record in the global staging slice with the normal recomputed per contact (the jammed phototaxis swarm: 472 rounds
// of ~1.8 k cycles per substep, 12 x slower per kilobot-step than the headline).  Round 3 sweeps it by DEPENDENCY DEPTH like the
// register path does its waves, but across the whole workgroup:
//   1. depth of every contact: one pass over the key buckets in canonical order (contacts of one key share no body);
//   2. counting sort of the contacts by depth INTO CONSECUTIVE RECORDS (pair, normal, impulse: 16 B, global scratch), so
//      that thread t of a round reads record [first of the level + t] -- coalesced, no indirection, and requested one level
//      ahead of the barrier that separates the levels;
//   3. warm start, velocity and position passes run level by level (the jammed swarm: 12 levels instead of ~22 keys).
// Conflicting contacts are met in the canonical order (a contact's level is 1 + the level of the latest earlier contact on
// either body), so the bits are those of the sequential sweep.
{
    unsigned *sPair_ = big ? gPair : lPair, *sInfo_ = big ? gInfo : lInfo;
    float *sAcc_ = big ? gAcc : lAcc;
    unsigned short *cbk_ = big ? gCbk : lCbk, *order_ = big ? gOrder : lOrder;
    // sorted records: 16 B per contact behind the staging records of all envs
    unsigned *sp2 = reinterpret_cast<unsigned *>(ka->buf.scratch) + (size_t)ka->E * ka->cap * 4 + wo * 4;
    float *snx = reinterpret_cast<float *>(sp2 + ka->cap), *sny = snx + ka->cap, *sacc2 = sny + ka->cap;
    // ... and their impulses in LDS: the pair array of the staging area is dead once the records are sorted (contacts staged in
    // the global slice: the whole LDS staging area, three arrays of capL words, is idle); envs beyond that keep them in the record
#ifndef KB_COOP_PD
#define KB_COOP_PD 4
#endif
#ifndef KB_COOP_ACC_LDS
#define KB_COOP_ACC_LDS 1
#endif
    const bool accInLds = KB_COOP_ACC_LDS && ncon <= (big ? 3 * capL_ : capL_);
    float *accL = reinterpret_cast<float *>(lPair);
    unsigned *bodyDepth = islCnt;       // zeroed by the bucket sort
    const int nlk = nList[0];
    // ---- 1. depth of every contact (kept in cbk) ----
    unsigned myMax = 0;
    if (tid == 0) misc[M_TOTAL] = 0;
    for (int li = 0; li < nlk; ++li) {
        const int bk = bkList[li];
        const int s_ = (int)bkStart[bk], e_ = (int)bkStart[bk + 1];
        const bool ranked = (bk % RK) == RK - 1;
        const int maxr_ = ranked ? (int)bkMaxRank[bk / RK] : RK - 1;
        for (int r_ = RK - 1; r_ <= maxr_; ++r_) {
            for (int i_ = s_ + tid; i_ < e_; i_ += nt) {
                const unsigned c = order_[i_];
                if (ranked && (int)((sInfo_[c] >> 8) & 0xFFu) != r_) continue;
                const unsigned pr = sPair_[c];
                const unsigned a = pr & 0xFFFFu, b = pr >> 16;
                const unsigned d = max(a < (unsigned)WALL_CODE ? bodyDepth[a] : 0u, bodyDepth[b]) + 1u;
                bodyDepth[b] = d;
                if (a < (unsigned)WALL_CODE) bodyDepth[a] = d;
                cbk_[c] = (unsigned short)d;
                myMax = max(myMax, d);
            }
            __syncthreads();
        }
    }
    KB_STAMP_PRE(19);    // (profile build, cumulative since the bucket sort) depth of every contact
    if (myMax) atomicMax(&misc[M_TOTAL], myMax);
    for (int k = tid; k < lds::nbk(nw) + 1; k += nt) { bkStart[k] = 0; if (k < lds::nbk(nw)) bkFill[k] = 0; }
    __syncthreads();
    const int maxD = (int)min(misc[M_TOTAL], (unsigned)lds::nbk(nw) - 2u);
    if (misc[M_TOTAL] > (unsigned)lds::nbk(nw) - 2u && tid == 0) atomicOr(&misc[M_STATUS], 4u);      // (a chain deeper than the level table: flagged, not bit-exact)
    // ---- 2. counting sort by depth into consecutive records ----
    for (int c = tid; c < ncon; c += nt) {
        const unsigned d = cbk_[c];
        if (d == (unsigned)EMPTY16 || d > (unsigned)maxD) continue;      // contact of a sleeping island: in no level
        atomicAdd(&bkStart[d], 1u);
    }
    __syncthreads();
    if (wave == 0) {      // exclusive scan of the level counts
        const int nb = maxD + 2;
        const int chunk = (nb + 63) / 64;
        const int s0 = lane * chunk, e0 = min(nb, s0 + chunk);
        unsigned sum = 0;
        for (int i = s0; i < e0; ++i) sum += bkStart[i];
        const unsigned incl = wave_incl_scan(sum);
        unsigned run = incl - sum;
        for (int i = s0; i < e0; ++i) { const unsigned v = bkStart[i]; bkStart[i] = run; run += v; }
    }
    __syncthreads();
    for (int c = tid; c < ncon; c += nt) {
        const unsigned d = cbk_[c];
        if (d == (unsigned)EMPTY16 || d > (unsigned)maxD) continue;
        const unsigned si = bkStart[d] + atomicAdd(&bkFill[d], 1u);
        const unsigned pr = sPair_[c], inf = sInfo_[c];
        const int a = (int)(pr & 0xFFFFu), b = (int)(pr >> 16);
        const bool flip = (inf & 0x80u) != 0u;
        // velocity-phase normal from the start-of-step positions (b2WorldManifold::Initialize)
        float nx = 1.0f, ny = 0.0f;
        if (a >= WALL_CODE) {
            float dist;
            wall_geom(ca, a - WALL_CODE, pos[b].x, pos[b].y, dist, nx, ny);
            if (flip) { nx = -nx; ny = -ny; }
        } else {
            const float dx = pos[b].x - pos[a].x, dy = pos[b].y - pos[a].y;
            const float dd = dx * dx + dy * dy;
            if (dd > B2_EPSILON * B2_EPSILON) {
                const float len = sqrtf(dd);
                const float inv = 1.0f / len;
                nx = dx * inv; ny = dy * inv;
            }
        }
        sp2[si] = (a >= WALL_CODE && flip) ? pr + 4u : pr;      // (wall contacts: body id WALL_CODE + wall + 4 * flipped)
        snx[si] = nx; sny[si] = ny; sacc2[si] = sAcc_[c];
        order_[si] = (unsigned short)c;
    }
    __syncthreads();
    if (accInLds) {      // (behind the barrier: the staged pairs have all been read)
        for (int si = tid; si < (int)bkStart[maxD + 1]; si += nt) accL[si] = sacc2[si];
        __syncthreads();
    }
    KB_STAMP_PRE(20);    // ... + counting sort by depth into consecutive records
    const int nsorted = (int)bkStart[maxD + 1];
    const float nm_bb = ca.nm_bb, nm_wb = ca.nm_wb;
    KB_ABLATE_EXIT(9);
    // ---- 3. warm start and velocity passes, level by level.  What a thread needs of a record never changes during the passes
    //         (pair, normal: 12 B), so it is requested PD levels ahead -- a round is shorter than a trip to L2 / HBM ----
    // (The impulses are read and written through a pointer of ONE address space per instantiation of the passes: a pointer that is
    //  "LDS or global" makes every access a FLAT instruction, which counts on the vector-memory counter too -- the round would
    //  then wait for ALL loads in flight, i.e. for the records requested PD levels ahead, and the prefetch would buy nothing.
    //  That was the state of the first version: ~ 1.3 k cycles per level.)
    auto vel_passes = [&](auto acc_in_lds_) __attribute__((always_inline)) {
        constexpr bool AL = decltype(acc_in_lds_)::value;
        constexpr int PD = KB_COOP_PD;
        const int nsteps = (ca.vel_iters + 1) * maxD;      // (pass, level) in sequence; pass 0 = b2ContactSolver::WarmStart
        unsigned rpr[PD];
        float rnx_[PD], rny_[PD];
        bool rhave[PD];
        int dreq = 0;      // level of the step that is requested next (1 .. maxD, wrapping from pass to pass)
        auto request = [&](int step_, unsigned &pr_, float &nx_, float &ny_, bool &have_) __attribute__((always_inline)) {
            // (every thread issues its three loads in every round, threads without a record of the level re-read record 0: with
            //  loads under a branch the compiler cannot count what is in flight, and the wait for the oldest request would again
            //  be a wait for all of them)
            dreq = dreq >= maxD ? 1 : dreq + 1;
            const int i_ = (int)bkStart[dreq] + tid;
            have_ = step_ < nsteps && i_ < (int)bkStart[dreq + 1];
            const int ic_ = have_ ? i_ : 0;
            pr_ = sp2[ic_]; nx_ = snx[ic_]; ny_ = sny[ic_];
        };
#pragma unroll
        for (int u = 0; u < PD; ++u) request(u, rpr[u], rnx_[u], rny_[u], rhave[u]);
        int d_ = 0;
        int nS = (int)bkStart[1], nE = (int)bkStart[2];      // bounds of the level that comes next: read one round ahead, with the round's other LDS reads
        for (int s0 = 0; s0 < nsteps; s0 += PD) {
#pragma unroll
            for (int u = 0; u < PD; ++u) {
                const int step_ = s0 + u;
                if (step_ >= nsteps) break;
                d_ = d_ >= maxD ? 1 : d_ + 1;
                const bool warm = step_ < maxD;
                const int e_ = nE;
                int ii = nS + tid;
                { const int nd = d_ >= maxD ? 1 : d_ + 1; nS = (int)bkStart[nd]; nE = (int)bkStart[nd + 1]; }
                // (the record of thread t comes out of the registers requested PD rounds ago; only a level with more contacts than
                //  threads reads further ones in place -- in a loop of its own, or the wait for "the record" would have to assume
                //  the youngest load and drain the whole request queue every round)
                auto one = [&](const unsigned pr, const float nx, const float ny, const int ii) __attribute__((always_inline)) {
                    const int a = (int)(pr & 0xFFFFu), b = (int)(pr >> 16);
                    const bool wallA = a >= WALL_CODE;
                    float acc;
                    if constexpr (AL) acc = accL[ii]; else acc = sacc2[ii];
                    if (warm) {
                        const float Px = acc * nx, Py = acc * ny;
                        if (!wallA) { vel[a].x -= ca.im_bot * Px; vel[a].y -= ca.im_bot * Py; }
                        vel[b].x += ca.im_bot * Px; vel[b].y += ca.im_bot * Py;
                    } else {
                        float vax = 0.0f, vay = 0.0f;
                        if (!wallA) { vax = vel[a].x; vay = vel[a].y; }
                        const float vbx = vel[b].x, vby = vel[b].y;
                        const float ima = wallA ? 0.0f : ca.im_bot, imb = ca.im_bot;
                        const float dvx = vbx - vax, dvy = vby - vay;
                        const float vn = dvx * nx + dvy * ny;
                        float lambda = -((wallA ? nm_wb : nm_bb) * vn);
                        const float newimp = fmaxf(acc + lambda, 0.0f);
                        lambda = newimp - acc;
                        if constexpr (AL) accL[ii] = newimp; else sacc2[ii] = newimp;
                        const float Px = lambda * nx, Py = lambda * ny;
                        if (!wallA) { vel[a].x = vax - ima * Px; vel[a].y = vay - ima * Py; }
                        vel[b].x = vbx + imb * Px; vel[b].y = vby + imb * Py;
                    }
                };
                if (rhave[u]) one(rpr[u], rnx_[u], rny_[u], ii);
                for (int i2 = ii + nt; i2 < e_; i2 += nt) {
                    const unsigned pr2 = sp2[i2];
                    const float nx2 = snx[i2], ny2 = sny[i2];
                    one(pr2, nx2, ny2, i2);
                }
                request(step_ + PD, rpr[u], rnx_[u], rny_[u], rhave[u]);
                lds_barrier();      // (velocities and impulses live in LDS; the requests stay in flight across the barrier)
            }
        }
    };
    if (accInLds) vel_passes(std::true_type{}); else vel_passes(std::false_type{});
#ifdef KB_PROFILE
    if (tid == 0) { atomicAdd(&KB_PROF(8), (unsigned)maxD); atomicAdd(&KB_PROF(11), 1u); }
#endif
    KB_STAMP(4);
    KB_RETID();
    KB_ABLATE_EXIT(11);
    // StoreImpulses: back to the staged contacts (their index is the position in the packed list)
    if (accInLds) { for (int si = tid; si < nsorted; si += nt) sAcc_[order_[si]] = accL[si]; }
    else {
        // (record si was last written by the thread that swept it in the final velocity pass, through GLOBAL memory, and this
        //  copy hands it to another thread: lds_barrier() orders LDS only, so the hand-over takes the barrier with the
        //  workgroup-scope release / acquire of the memory model -- block-uniform, once per substep, only with the impulses
        //  in the records.  On gfx950 it compiles to the same s_waitcnt lgkmcnt(0) + s_barrier: vector memory of one
        //  workgroup is ordered by the CU's in-order L1, DESIGN.md 3)
        __syncthreads();
        for (int si = tid; si < nsorted; si += nt) sAcc_[order_[si]] = sacc2[si];
    }
    // integrate positions (b2Island::Solve)
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        const int b_ = tid + q * nt;
        if (b_ >= N) continue;
        const int b = ms[q];
        float vxx = vel[b].x, vyy = vel[b].y, ww = bw[q];
        startX[b] = pos[b].x; startY[b] = pos[b].y;     // pose at the start of the substep (continuous step)
        const float tx = h * vxx, ty = h * vyy;
        if (tx * tx + ty * ty > B2_MAX_TRANSLATION_SQ) {
            const float ratio = B2_MAX_TRANSLATION / sqrtf(tx * tx + ty * ty);
            vxx *= ratio; vyy *= ratio;
        }
        const float rot = h * ww;
        if (rot * rot > B2_MAX_ROTATION_SQ) {
            const float ratio = B2_MAX_ROTATION / fabsf(rot);
            ww *= ratio;
        }
        pos[b].x += h * vxx; pos[b].y += h * vyy;
        th[q] += h * ww;
        vel[b].x = vxx; vel[b].y = vyy; bw[q] = ww;
        if (SLEEP) islWave[b] = (unsigned char)((active[b] ? 2 : 0) | (ca.pos_iters <= 0 ? 1 : 0));
    }
    __syncthreads();
    KB_STAMP(5);
    KB_RETID();
    KB_ABLATE_EXIT(12);
    // SolvePositionConstraints; an island stops once its minSeparation >= -3 slop.  The pair of thread t in a level is requested
    // PD levels ahead here as well (wrapping into the next iteration; a request too many is only a load).
    {
        constexpr int PD = 4;
        const int posIters = ca.pos_iters;      // (phase-scoped arguments: loaded in front of the sweeps)
        unsigned rpr[PD];
        bool rhave[PD];
        int dreq = 0;
        auto request = [&](unsigned &pr_, bool &have_) __attribute__((always_inline)) {
            dreq = dreq >= maxD ? 1 : dreq + 1;      // (branch-free, as in the velocity passes)
            const int i_ = (int)bkStart[dreq] + tid;
            have_ = maxD > 0 && i_ < (int)bkStart[dreq + 1];
            pr_ = sp2[have_ ? i_ : 0];
        };
#pragma unroll
        for (int u = 0; u < PD; ++u) request(rpr[u], rhave[u]);
        int d_ = 0, u_ = 0;      // u_: which of the PD request registers holds the current level
        int nS = maxD > 0 ? (int)bkStart[1] : 0, nE = maxD > 0 ? (int)bkStart[2] : 0;
        for (int it = 0; it < posIters; ++it) {
            unsigned char *act = active + (it & 1) * NB, *nxt = active + ((it + 1) & 1) * NB;
            bool viol = false;
            for (int lv = 0; lv < maxD; ++lv) {
                d_ = d_ >= maxD ? 1 : d_ + 1;
                const int e_ = nE;
                int ii = nS + tid;
                { const int nd = d_ >= maxD ? 1 : d_ + 1; nS = (int)bkStart[nd]; nE = (int)bkStart[nd + 1]; }
                // (the request registers are a ring; the ring index is uniform, the selects are a handful of moves)
                const bool have = u_ == 0 ? rhave[0] : (u_ == 1 ? rhave[1] : (u_ == 2 ? rhave[2] : rhave[3]));
                const unsigned pr0 = u_ == 0 ? rpr[0] : (u_ == 1 ? rpr[1] : (u_ == 2 ? rpr[2] : rpr[3]));
                auto one = [&](const unsigned pr) __attribute__((always_inline)) {
                    const int a = (int)(pr & 0xFFFFu);
                    const int b = (int)(pr >> 16);
                    const int isl = (int)parent[b];
                    if (act[isl]) {
                        float nx, ny, sep;
                        const float ima = a < WALL_CODE ? ca.im_bot : 0.0f, imb = ca.im_bot;
                        const float bx = pos[b].x, by = pos[b].y;
                        float axx = 0.0f, ayy = 0.0f;
                        if (a >= WALL_CODE) {
                            const bool flipped = a >= WALL_CODE + 4;      // manifold normal fixed at detection
                            float dist, wx, wy;
                            wall_geom(ca, (a - WALL_CODE) & 3, bx, by, dist, wx, wy);
                            nx = flipped ? -wx : wx; ny = flipped ? -wy : wy;
                            const float along = flipped ? -dist : dist;
                            sep = along - B2_POLYGON_RADIUS - ca.r_bot;
                        } else {
                            axx = pos[a].x; ayy = pos[a].y;
                            const float dx = bx - axx, dy = by - ayy;
                            const float len = sqrtf(dx * dx + dy * dy);
                            nx = dx; ny = dy;
                            if (!(len < B2_EPSILON)) { const float inv = 1.0f / len; nx = dx * inv; ny = dy * inv; }
                            sep = (dx * nx + dy * ny) - ca.r_bot - ca.r_bot;
                        }
                        if (sep < -3.0f * B2_LINEAR_SLOP) { nxt[isl] = 1; viol = true; if (SLEEP && it == posIters - 1) islWave[isl] = 3; }
                        const float C = kb_clampf(B2_BAUMGARTE * (sep + B2_LINEAR_SLOP), -B2_MAX_LINEAR_CORRECTION, 0.0f);
                        const float K = ima + imb;
                        const float imp = K > 0.0f ? -C / K : 0.0f;
                        const float Px = imp * nx, Py = imp * ny;
                        if (a < WALL_CODE) { pos[a].x = axx - ima * Px; pos[a].y = ayy - ima * Py; }
                        pos[b].x = bx + imb * Px; pos[b].y = by + imb * Py;
                    }
                };
                if (have) one(pr0);      // (the requested record; further ones of a level with more contacts than threads in a loop of their own, see above)
                for (int i2 = ii + nt; i2 < e_; i2 += nt) { const unsigned pr2 = sp2[i2]; one(pr2); }
                {   // request the level PD steps ahead into the register that has just been used
                    unsigned npr; bool nhave;
                    request(npr, nhave);
                    if (u_ == 0) { rpr[0] = npr; rhave[0] = nhave; } else if (u_ == 1) { rpr[1] = npr; rhave[1] = nhave; }
                    else if (u_ == 2) { rpr[2] = npr; rhave[2] = nhave; } else { rpr[3] = npr; rhave[3] = nhave; }
                    u_ = (u_ + 1) & (PD - 1);
                }
                lds_barrier();
            }
            if (viol) misc[M_ANY] = 1u;
            __syncthreads();
            const bool any = misc[M_ANY] != 0u;
            __syncthreads();
            if (tid == 0) misc[M_ANY] = 0u;
            if (!any) break;
            // the flags the next sweep sets must start cleared
            for (int si = tid; si < nsorted; si += nt) act[parent[sp2[si] >> 16]] = 0;
            __syncthreads();
        }
    }
}
