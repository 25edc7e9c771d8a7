// kb_regsolve_bins.inc -- register-resident solver of the kernels without objects (textually included by kb_step_kernel.h
// inside the substep loop; every name it uses is a local of the kernel).
//
// Round 3: the sweeps are VALU-issue-bound (tools/phase_ablation.py: the ten velocity sweeps were 26 % of a launch and 30 % of
// its vector instructions), and a sweep round costs the same whether 13 or 64 of a wave's lanes hold a contact of the level.
// So only the first `nsolve` waves of the workgroup (half of them) sweep, each with up to KRB = 4 contacts per lane: the
// islands are placed on fewer waves, a depth level fills more lanes of a round, and the other waves wait at the barrier
// without issuing anything.  A contact costs five registers: the pair of bodies, one word of bookkeeping
// (staging index | depth level | normal flipped | island root), the accumulated impulse and the normal -- inverse masses,
// radii and effective masses follow from "is A a wall".  Same arithmetic, same order of operations as the two-slot solver
// of the kernels with objects (below in kb_step_kernel.h): the canonical Gauss-Seidel order by dependency depth.
{
    constexpr int KRB = KB_KREG_BINS;
    const bool solving = (int)__builtin_amdgcn_readfirstlane(wave) < nsolve;
    // per contact: LDS byte offsets of its two bodies inside the float2 body arrays (a wall is one of four bodies at rest behind
    // the kilobots: velocity (0, 0), inverse mass 0 -- the sweeps need no second code path for it);  staging index (12) |
    // depth (9) << 12 | flipped << 21 | island root << 22;  accumulated impulse;  normal
    unsigned ra[KRB], rb[KRB], rm[KRB];
    float racc[KRB];
    kb_pair rn[KRB];       // (x, y) in one aligned register pair: the rounds below work on pairs, see kb_common.h
    const unsigned WOFF = 8u * (unsigned)(NB - 5);
    char *const velB = reinterpret_cast<char *>(vel), *const posB = reinterpret_cast<char *>(pos);
#define RB_WALL(j) (ra[j] >= WOFF)
#define RB_WALLIDX(j) ((int)((ra[j] - WOFF) >> 3))
#define RB_VEL(off) (*reinterpret_cast<float2 *>(velB + (off)))
#define RB_POS(off) (*reinterpret_cast<float2 *>(posB + (off)))
#define RB_C(j) ((int)(rm[j] & 0xFFFu))
#define RB_DEPTH(j) ((int)((rm[j] >> 12) & 0x1FFu))
#define RB_FLIP(j) (((rm[j] >> 21) & 1u) != 0u)
#define RB_ISL(j) ((int)(rm[j] >> 22))
#pragma unroll
    for (int j = 0; j < KRB; ++j) { ra[j] = 0u; rb[j] = 0u; rm[j] = 0u; racc[j] = 0.0f; rn[j] = kb_pair{1.0f, 0.0f}; }
    unsigned long long slotLevels[KRB];
    int dlo[KRB], dhi[KRB];         // levels of the slot's contacts (wave-uniform)
#pragma unroll
    for (int j = 0; j < KRB; ++j) { slotLevels[j] = 0ull; dlo[j] = 1; dhi[j] = 0; }
    int maxD = 0;
    unsigned mycnt = 0;
    bool twoSlot = false;           // (wave-uniform) the wave holds more than 64 contacts
    // (phase-scoped arguments: `ca` was loaded in front of the barrier that opens the solver; nothing from here to the end of the
    //  position sweeps reads the argument segment, so no wave's chain waits for scalar memory)
    const float nm_bb = ca.nm_bb, nm_wb = ca.nm_wb;
    const int velIters = ca.vel_iters, posIters = ca.pos_iters;
#ifdef KB_SOLVER_PRIO
    __builtin_amdgcn_s_setprio(KB_SOLVER_PRIO);     // the serial chain of the substep: ahead of the other envs' throughput phases
#endif
    if (solving) {
        // ---- light load: bodies and key of the contacts of this wave, in arrival order.  The grouping pass left the wave's fill
        // pointer at the end of its stretch of lOrder, so the stretch is two words read side by side. ----
        mycnt = misc[M_WCNT + wave];
        const unsigned mybase = misc[M_WFILL + wave] - mycnt;
        // A wave of at most 64 contacts -- since the packed placement most waves of an env, the deep ones among them -- holds
        // nothing behind slot 0: it takes the one-slot set-up below.  The test is scalar and picks a whole version of every
        // trip, so in a two-slot wave both slots still issue their loads together.
        twoSlot = KB_SETUP_FUSED == 0 || (unsigned)__builtin_amdgcn_readfirstlane((int)mycnt) > 64u;
        if (twoSlot) {
            unsigned lk[KRB];          // key (6) | rank (8) << 8 | staging index << 16 | valid << 31;  key 63: contact of a sleeping island
            unsigned lp[KRB];           // a | b << 16 (body indices; a wall is WALL_CODE + w)
            int rdepth[KRB];
            unsigned klo[KRB], khi[KRB];    // the slot's key as a bit (none: no contact, or one of a sleeping island)
#define RB_A(j) ((int)(lp[j] & 0xFFFFu))
#define RB_B(j) ((int)(lp[j] >> 16))
            // Both slots go through every trip together: the lanes without a contact read entry 0 and drop what they get, so no
            // slot waits under a branch of its own for the slot in front of it (as in label_pass_bins).
            {
                unsigned c_[KRB], inf_[KRB];
                bool v_[KRB], awake_[KRB];
#pragma unroll
                for (int j = 0; j < KRB; ++j) {
                    const unsigned idx = lane + 64u * j;
                    v_[j] = idx < mycnt;
                    c_[j] = lOrder[v_[j] ? mybase + idx : 0u];
                }
#pragma unroll
                for (int j = 0; j < KRB; ++j) {
                    c_[j] = v_[j] ? c_[j] : 0u;
                    lp[j] = lPair[c_[j]]; inf_[j] = lInfo[c_[j]];
                }
#pragma unroll
                for (int j = 0; j < KRB; ++j) { lp[j] = v_[j] ? lp[j] : 0u; awake_[j] = true; }
                if (SLEEP) {
                    unsigned root_[KRB];
#pragma unroll
                    for (int j = 0; j < KRB; ++j) root_[j] = parent[lp[j] >> 16];
#pragma unroll
                    for (int j = 0; j < KRB; ++j) awake_[j] = active[root_[j]] != 0;
                }
#pragma unroll
                for (int j = 0; j < KRB; ++j) {
                    const unsigned cls = inf_[j] & 0x7Fu, r = (inf_[j] >> 8) & 0xFFu;
                    unsigned key = cls * RK + (r < RK - 1 ? r : RK - 1);
                    const bool on = v_[j] && awake_[j];
                    if (!on) key = 63u;     // in no round (depth 0), its impulse is carried over
                    const unsigned bit = on ? 1u << (key & 31u) : 0u;
                    klo[j] = key < 32u ? bit : 0u; khi[j] = key < 32u ? 0u : bit;
                    if (on && r >= RK - 1) atomicMax(&bkMaxRank[wave * NUM_CLS + cls], r);
                    lk[j] = v_[j] ? (key | (r << 8) | (c_[j] << 16) | 0x80000000u) : 0u;
                    rdepth[j] = 0;
                }
            }
            // keys present in the wave, and those of them that the slots behind slot 0 hold as well (wave-uniform)
            unsigned long long keymask = 0ull, restmask = 0ull;
            {
                unsigned mlo = 0, mhi = 0, rlo = 0, rhi = 0;
#pragma unroll
                for (int j = 0; j < KRB; ++j) { mlo |= klo[j]; mhi |= khi[j]; if (j > 0) { rlo |= klo[j]; rhi |= khi[j]; } }
                mlo = wave_or(mlo); mhi = wave_or(mhi);
                keymask = ((unsigned long long)mhi << 32) | mlo;
                if (mycnt > 64u) { rlo = wave_or(rlo); rhi = wave_or(rhi); restmask = ((unsigned long long)rhi << 32) | rlo; }
            }
            wave_sync();   // bkMaxRank of this wave
#ifdef KB_PROFILE
            if (tid == 0) { atomicAdd(&KB_PROF(8), (unsigned)__popcll(keymask)); atomicAdd(&KB_PROF(11), 1u); }
#endif
            KB_STAMP_PRE(19);    // (profile build) wave 0: contacts grouped + light load
            // ---- dependency depth of every contact: 1 + the depth of the latest earlier contact (canonical key order) on either
            // of its bodies.  Contacts of equal depth never share a body, and sweeping by increasing depth keeps the relative
            // order of any two contacts that do -- so depth rounds give exactly the result of the key-by-key sweep. ----
            unsigned *bodyDepth = islCnt;   // zeroed before the contacts were grouped
            {
                // A round is one LDS trip under the EXEC mask of the lanes whose contact is of the round: the round a contact
                // belongs to (its key; in the open-ended rank bucket its key and rank) and the addresses of its two bodies are
                // made once, a wall contact names its kilobot twice (max(d, d) + 1: the wall has no depth), a slot without a
                // contact of the key is left out by a scalar test, and the highest ranks of the wave's open-ended buckets are
                // fetched once, one class per lane.
                char *const bdB = reinterpret_cast<char *>(bodyDepth);
#define RB_BD(off) (*reinterpret_cast<unsigned *>(bdB + (off)))
                unsigned rc[KRB], ia4[KRB], ib4[KRB];
#pragma unroll
                for (int j = 0; j < KRB; ++j) {
                    const unsigned key = lk[j] & 63u, r = (lk[j] >> 8) & 0xFFu;
                    const bool on = (lk[j] >> 31) != 0u && key != 63u;
                    rc[j] = on ? ((key % RK) == RK - 1 ? (key | (r << 6)) : key) : 0xFFFFFFFFu;
                    ib4[j] = 4u * (unsigned)RB_B(j);
                    ia4[j] = RB_A(j) < WALL_CODE ? 4u * (unsigned)RB_A(j) : ib4[j];
                }
                const unsigned mrow = bkMaxRank[wave * NUM_CLS + min((int)lane, NUM_CLS - 1)];
                for (unsigned long long m_ = keymask; m_; m_ &= m_ - 1) {
                    const unsigned key_ = (unsigned)__builtin_ctzll(m_);
                    const bool rest_ = ((restmask >> key_) & 1ull) != 0ull;
                    auto depth_round = [&](unsigned code_) __attribute__((always_inline)) {
                        // (the contacts of a round share no body: the slots may go one after the other)
#pragma unroll
                        for (int j = 0; j < KRB; ++j) {
                            if (j == 0 || rest_) {
                                if (rc[j] == code_) {
                                    const unsigned d = max(RB_BD(ia4[j]), RB_BD(ib4[j])) + 1u;
                                    rdepth[j] = (int)d;
                                    RB_BD(ib4[j]) = d;
                                    RB_BD(ia4[j]) = d;
                                }
                            }
                        }
                        wave_sync();
                    };
                    if ((key_ % RK) < RK - 1) depth_round(key_);
                    else {
                        const unsigned maxr_ = (unsigned)__builtin_amdgcn_readlane((int)mrow, (int)(key_ / RK));
                        for (unsigned r_ = RK - 1; r_ <= maxr_; ++r_) depth_round(key_ | (r_ << 6));
                    }
                }
#undef RB_BD
            }
#pragma unroll
            for (int j = 0; j < KRB; ++j) maxD = max(maxD, rdepth[j]);
            maxD = (int)wave_umax((unsigned)maxD);
            KB_STAMP_PRE(20);    // ... + depth pass
            // ---- deal the contacts to (lane, slot) in order of depth: the 64 shallowest go to slot 0, the next 64 to slot 1, ...
            // A depth level then lives in one slot (two at a boundary), and a round only pays for the slots that hold contacts
            // of its level. ----
            if (mycnt > 64u) {
                // the place of every contact first (ballots and lane counts, nothing waits for memory), then one write per slot,
                // and both slots read back side by side
                unsigned at[KRB];
#pragma unroll
                for (int j = 0; j < KRB; ++j) at[j] = 0u;
                unsigned base_ = 0;
                for (int d_ = SLEEP ? 0 : 1; d_ <= maxD; ++d_) {      // (depth 0: contacts of sleeping islands)
#pragma unroll
                    for (int j = 0; j < KRB; ++j) {
                        const bool is = (lk[j] >> 31) && rdepth[j] == d_;
                        const unsigned long long m_ = __ballot(is);
                        const unsigned mine = __builtin_amdgcn_mbcnt_hi((unsigned)(m_ >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_, base_));
                        at[j] = is ? mine : at[j];
                        base_ += (unsigned)__popcll(m_);
                    }
                }
#pragma unroll
                for (int j = 0; j < KRB; ++j)
                    if (lk[j] >> 31) {
                        lOrder[mybase + at[j]] = (unsigned short)((lk[j] >> 16) & 0xFFFu);
                        lCbk[mybase + at[j]] = (unsigned short)rdepth[j];
                    }
                wave_sync();
                unsigned short o_[KRB], l_[KRB];
#pragma unroll
                for (int j = 0; j < KRB; ++j) {
                    const unsigned i_ = mybase + ((lk[j] >> 31) ? lane + 64u * j : 0u);
                    o_[j] = lOrder[i_]; l_[j] = lCbk[i_];
                }
#pragma unroll
                for (int j = 0; j < KRB; ++j) {
                    const bool v_ = (lk[j] >> 31) != 0u;
                    lk[j] = v_ ? ((lk[j] & 0x8000FFFFu) | ((unsigned)o_[j] << 16)) : lk[j];
                    rdepth[j] = v_ ? (int)l_[j] : rdepth[j];
                }
            }
            KB_STAMP_PRE(21);    // ... + dealing
            // depth levels present in every slot (bit min(depth, 63)), wave-uniform
#pragma unroll
            for (int j = 0; j < KRB; ++j) {
                const unsigned long long mine = (lk[j] >> 31) ? 1ull << min(rdepth[j], 63) : 0ull;
                const unsigned lo = wave_or((unsigned)mine), hi = wave_or((unsigned)(mine >> 32));
                slotLevels[j] = ((unsigned long long)hi << 32) | (unsigned long long)lo;
                // the levels of a slot are a contiguous range (the dealing above; without it everything sits in slot 0), and the
                // ranges of successive slots follow each other: a sweep is slot 0's levels in order, then slot 1's, ... --
                // contacts of one level never share a body, so a level split over two slots may run in two rounds.
                const unsigned long long lv = slotLevels[j] >> 1;      // (level 0: contacts of sleeping islands, in no round)
                dlo[j] = lv ? (int)__builtin_ctzll(lv) + 1 : 1;
                dhi[j] = lv ? ((lv >> 62) ? maxD : 64 - (int)__builtin_clzll(lv)) : 0;
            }
            // ---- full load of the contacts ----
            // Two trips for both slots together: the contact's words, then its bodies.  The lanes without a contact load
            // contact 0 and body 0 and keep the idle record (no bodies, no impulse, normal (1, 0)).
            {
                unsigned c_[KRB], pr_[KRB], inf_[KRB], root_[KRB];
                float acc_[KRB];
                float2 pa_[KRB], pb_[KRB];
                bool v_[KRB];
#pragma unroll
                for (int j = 0; j < KRB; ++j) {
                    v_[j] = (lk[j] >> 31) != 0u;
                    c_[j] = v_[j] ? (lk[j] >> 16) & 0xFFFu : 0u;
                    pr_[j] = lPair[c_[j]]; inf_[j] = lInfo[c_[j]]; acc_[j] = lAcc[c_[j]];
                }
#pragma unroll
                for (int j = 0; j < KRB; ++j) {
                    pr_[j] = v_[j] ? pr_[j] : 0u;
                    const int a = (int)(pr_[j] & 0xFFFFu), b = (int)(pr_[j] >> 16);
                    pa_[j] = pos[a >= WALL_CODE ? b : a]; pb_[j] = pos[b]; root_[j] = parent[b];
                }
                bool pairOn[KRB];
                kb_pair d_[KRB];
                float dd[KRB], wnx[KRB], wny[KRB];
                bool ieee = false;
#pragma unroll
                for (int j = 0; j < KRB; ++j) {
                    const int a = (int)(pr_[j] & 0xFFFFu), b = (int)(pr_[j] >> 16);
                    const bool wallA = a >= WALL_CODE, flip = (inf_[j] & 0x80u) != 0u;
                    ra[j] = wallA ? WOFF + 8u * (unsigned)(a - WALL_CODE) : 8u * (unsigned)a;
                    rb[j] = 8u * (unsigned)b;
                    racc[j] = v_[j] ? acc_[j] : 0.0f;
                    rm[j] = v_[j] ? (c_[j] | ((unsigned)rdepth[j] << 12) | (flip ? 1u << 21 : 0u) | (root_[j] << 22)) : 0u;
                    // velocity-phase normal from the start-of-step positions (b2WorldManifold::Initialize)
                    float dist;
                    wall_geom(ca, wallA ? a - WALL_CODE : 0, pb_[j].x, pb_[j].y, dist, wnx[j], wny[j]);
                    if (flip) { wnx[j] = -wnx[j]; wny[j] = -wny[j]; }
                    d_[j] = pk_load(pb_[j]) - pk_load(pa_[j]);
                    dd[j] = pk_dot(d_[j], d_[j]);
                    pairOn[j] = v_[j] && !wallA && dd[j] > B2_EPSILON * B2_EPSILON;
                    ieee = ieee || (pairOn[j] && !kb_exact_guard(dd[j]));
                    rn[j] = wallA ? kb_pair{wnx[j], wny[j]} : kb_pair{1.0f, 0.0f};
                }
                // the IEEE sequences of sqrtf and the division are two dozen dependent instructions; with every pair of the wave
                // inside the proven range one correction step on the hardware seeds gives the same bits (kb_exact.h)
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(ieee) == 0ull, 1)) {
#pragma unroll
                    for (int j = 0; j < KRB; ++j) {
                        const float len = kb_sqrt_refine(dd[j], __builtin_amdgcn_sqrtf(dd[j]), __builtin_amdgcn_rsqf(dd[j]));
                        const float inv = kb_rcp_refine(len, __builtin_amdgcn_rcpf(len));
                        if (pairOn[j]) rn[j] = d_[j] * pk_splat(inv);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < KRB; ++j) {
                        const float len = sqrtf(dd[j]);
                        const float inv = 1.0f / len;
                        if (pairOn[j]) rn[j] = d_[j] * pk_splat(inv);
                    }
                }
            }
#undef RB_A
#undef RB_B
        } else {
            // ---- one-slot wave: slot 1 keeps the idle record it starts with -- none of its loads, keys, masks, levels,
            // geometry or refinements is issued -- and slot 0 is loaded once, in arrival order (nothing is dealt), in three
            // trips in front of the depth pass: lOrder;  the contact's words;  its bodies.  The depth field of rm is filled by
            // the round that assigns it, so nothing is read again behind the depth pass. ----
            const bool v_ = lane < mycnt;
            unsigned c_ = lOrder[v_ ? mybase + lane : 0u];
            c_ = v_ ? c_ : 0u;
            unsigned pr_ = lPair[c_];
            const unsigned inf_ = lInfo[c_];
            const float acc_ = lAcc[c_];
            pr_ = v_ ? pr_ : 0u;
            const int a = (int)(pr_ & 0xFFFFu), b = (int)(pr_ >> 16);
            const bool wallA = a >= WALL_CODE, flip = (inf_ & 0x80u) != 0u;
            const float2 pa_ = pos[wallA ? b : a], pb_ = pos[b];
            const unsigned root_ = parent[b];
            bool awake_ = true;
            if (SLEEP) awake_ = active[root_] != 0;
            // the round of the contact: its key, in the open-ended rank bucket its key and rank (none: no contact, or one of a
            // sleeping island -- key 63, in no round, depth 0, its impulse is carried over)
            const unsigned cls = inf_ & 0x7Fu, r = (inf_ >> 8) & 0xFFu;
            const unsigned key = cls * RK + (r < RK - 1 ? r : RK - 1);
            const bool on = v_ && awake_;
            if (on && r >= RK - 1) atomicMax(&bkMaxRank[wave * NUM_CLS + cls], r);
            const unsigned rc = on ? (r >= RK - 1 ? (key | (r << 6)) : key) : 0xFFFFFFFFu;
            const unsigned bit = on ? 1u << (key & 31u) : 0u;
            const unsigned long long keymask = ((unsigned long long)wave_or(key < 32u ? 0u : bit) << 32) | wave_or(key < 32u ? bit : 0u);
            // the record, as the full load of a two-slot wave makes it
            ra[0] = wallA ? WOFF + 8u * (unsigned)(a - WALL_CODE) : 8u * (unsigned)a;
            rb[0] = 8u * (unsigned)b;
            racc[0] = v_ ? acc_ : 0.0f;
            rm[0] = v_ ? (c_ | (flip ? 1u << 21 : 0u) | (root_ << 22)) : 0u;
            {
                // velocity-phase normal from the start-of-step positions (b2WorldManifold::Initialize)
                float dist, wnx, wny;
                wall_geom(ca, wallA ? a - WALL_CODE : 0, pb_.x, pb_.y, dist, wnx, wny);
                if (flip) { wnx = -wnx; wny = -wny; }
                const kb_pair d_ = pk_load(pb_) - pk_load(pa_);
                const float dd = pk_dot(d_, d_);
                const bool pairOn = v_ && !wallA && dd > B2_EPSILON * B2_EPSILON;
                rn[0] = wallA ? kb_pair{wnx, wny} : kb_pair{1.0f, 0.0f};
                // (one correction step on the hardware seeds where every pair of the wave is inside the proven range: kb_exact.h)
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(pairOn && !kb_exact_guard(dd)) == 0ull, 1)) {
                    const float len = kb_sqrt_refine(dd, __builtin_amdgcn_sqrtf(dd), __builtin_amdgcn_rsqf(dd));
                    const float inv = kb_rcp_refine(len, __builtin_amdgcn_rcpf(len));
                    if (pairOn) rn[0] = d_ * pk_splat(inv);
                } else {
                    const float len = sqrtf(dd);
                    const float inv = 1.0f / len;
                    if (pairOn) rn[0] = d_ * pk_splat(inv);
                }
            }
            wave_sync();   // bkMaxRank of this wave
#ifdef KB_PROFILE
            if (tid == 0) { atomicAdd(&KB_PROF(8), (unsigned)__popcll(keymask)); atomicAdd(&KB_PROF(11), 1u); }
#endif
            KB_STAMP_PRE(19);    // (profile build) wave 0: contacts grouped + load
            // ---- depth pass, as in a two-slot wave: one round per key present in the wave, in canonical order.  That is the
            // order of b2ContactSolver::WarmStart, the contacts of a round share no body, and a contact's impulse acc * n depends
            // on nothing another contact writes: every body sees the same sequence of v -+ im * P whether the warm start goes
            // key by key or rides in these rounds.  So a lane whose contact is of the round also warm-starts its two bodies:
            // two more reads beside the bodyDepth words, two more writes, the same trip -- and no warm-start pass of its own.
            // (The expressions are those of the pass below: a wall is a body at rest with inverse mass 0.) ----
            {
                char *const bdB = reinterpret_cast<char *>(islCnt);     // bodyDepth: zeroed before the contacts were grouped
#define RB_BD(off) (*reinterpret_cast<unsigned *>(bdB + (off)))
                const unsigned ib4 = rb[0] >> 1, ia4 = wallA ? ib4 : ra[0] >> 1;       // (a wall has no depth: max(d, d) + 1)
                const kb_pair P = pk_splat(racc[0]) * rn[0];
                const float ima = wallA ? 0.0f : ca.im_bot;
                const kb_pair da = pk_splat(ima) * P, db = pk_splat(ca.im_bot) * P;
                const unsigned mrow = bkMaxRank[wave * NUM_CLS + min((int)lane, NUM_CLS - 1)];
                unsigned depth_ = 0;
                for (unsigned long long m_ = keymask; m_; m_ &= m_ - 1) {
                    const unsigned key_ = (unsigned)__builtin_ctzll(m_);
                    auto depth_round = [&](unsigned code_) __attribute__((always_inline)) {
                        if (rc == code_) {
                            const unsigned d = max(RB_BD(ia4), RB_BD(ib4)) + 1u;
                            if (KB_SETUP_FUSED >= 2) {
                                const kb_pair va = pk_load(RB_VEL(ra[0])), vb = pk_load(RB_VEL(rb[0]));
                                RB_VEL(ra[0]) = pk_store(va - da);
                                RB_VEL(rb[0]) = pk_store(vb + db);
                            }
                            depth_ = d;
                            RB_BD(ib4) = d;
                            RB_BD(ia4) = d;
                        }
                        wave_sync();
                    };
                    if ((key_ % RK) < RK - 1) depth_round(key_);
                    else {
                        const unsigned maxr_ = (unsigned)__builtin_amdgcn_readlane((int)mrow, (int)(key_ / RK));
                        for (unsigned r_ = RK - 1; r_ <= maxr_; ++r_) depth_round(key_ | (r_ << 6));
                    }
                }
#undef RB_BD
                rm[0] |= depth_ << 12;
                maxD = (int)wave_umax(depth_);
                KB_STAMP_PRE(20);    // ... + depth pass with the warm start in its rounds
                KB_STAMP_PRE(21);    // (nothing is dealt)
                // depth levels present in slot 0 (bit min(depth, 63)); slot 1 holds none
                const unsigned long long mine = v_ ? 1ull << min(depth_, 63u) : 0ull;
                slotLevels[0] = ((unsigned long long)wave_or((unsigned)(mine >> 32)) << 32) | (unsigned long long)wave_or((unsigned)mine);
                const unsigned long long lv = slotLevels[0] >> 1;      // (level 0: contacts of sleeping islands, in no round)
                dlo[0] = lv ? (int)__builtin_ctzll(lv) + 1 : 1;
                dhi[0] = lv ? ((lv >> 62) ? maxD : 64 - (int)__builtin_clzll(lv)) : 0;
            }
        }
#ifdef KB_PROFILE
        if (lane == 0) atomicMax(&misc[M_PROF], (unsigned)maxD);
        if (tid == 0) atomicAdd(&KB_PROF(M_PROF_DEPTH), (unsigned)maxD);
        {
            // waves of the env that hold two slots (word 36), and the rounds one sweep of this wave runs -- a level split over
            // the two slots is swept twice -- as a maximum over the env's waves (word 38, added up in word 37 behind the
            // barrier at the end of the position sweeps) and for wave 0 (word 39); words from 13 on go out in units of 16
            unsigned rounds_ = 0;
#pragma unroll
            for (int j = 0; j < KRB; ++j) rounds_ += dhi[j] >= dlo[j] ? (unsigned)(dhi[j] - dlo[j] + 1) : 0u;
            if (lane == 0) { if (mycnt > 64u) atomicAdd(&KB_PROF(36), 16u); atomicMax(&KB_PROF(38), rounds_); }
            if (tid == 0) atomicAdd(&KB_PROF(39), 16u * rounds_);
        }
        KB_STAMP(7);    // register load + depth sweep of wave 0 (no barrier: wave-local time)
#endif
    }
    KB_ABLATE_EXIT(9);     // register set-up: light load, depth pass, dealing, full load -- and the warm start of the one-slot waves
    // one round of a sweep on slot j: the contacts of depth level d_ (a contact with depth 0 -- none, or of a sleeping island -- is in no round)
#define RB_ON(j) (RB_DEPTH(j) == d_)
    if (solving) {
        // b2ContactSolver::WarmStart of the two-slot waves, level by level (a one-slot wave has done it in its depth rounds)
        if (twoSlot || KB_SETUP_FUSED < 2) {
#pragma unroll
            for (int j = 0; j < KRB; ++j) {
                for (int d_ = dlo[j]; d_ <= dhi[j]; ++d_) {
                    if (RB_ON(j)) {
                        const kb_pair va = pk_load(RB_VEL(ra[j])), vb = pk_load(RB_VEL(rb[j]));
                        const kb_pair P = pk_splat(racc[j]) * rn[j];
                        const float ima = RB_WALL(j) ? 0.0f : ca.im_bot;
                        RB_VEL(ra[j]) = pk_store(va - pk_splat(ima) * P);
                        RB_VEL(rb[j]) = pk_store(vb + pk_splat(ca.im_bot) * P);
                    }
                    wave_sync();
                }
            }
        }
        KB_STAMP_PRE(29);    // (profile build) warm-start pass of wave 0, since the register set-up (a one-slot wave: nothing left to do)
    }
    KB_ABLATE_EXIT(10);    // warm-start pass of the two-slot waves
    if (solving) {
        // SolveVelocityConstraints: friction 0, restitution 0, one manifold point.  Only the lanes whose contact is of the round's
        // level execute (EXEC mask); a wall is a body at rest with inverse mass 0 (its "velocity" is rewritten as 0 - 0 * P).
        for (int it = 0; it < velIters; ++it) {
#pragma unroll
            for (int j = 0; j < KRB; ++j) {
                for (int d_ = dlo[j]; d_ <= dhi[j]; ++d_) {
                    if (RB_ON(j)) {
                        // (every line on a pair is one packed instruction for both components; the order of operations of each
                        //  component is the scalar one: dv . n as two products and their sum, v -+ im * (lambda * n))
                        const kb_pair va = pk_load(RB_VEL(ra[j])), vb = pk_load(RB_VEL(rb[j]));
                        const bool wallA = RB_WALL(j);
                        const kb_pair n = rn[j];
                        const float ima = wallA ? 0.0f : ca.im_bot, imb = ca.im_bot;
                        const float vn = pk_dot(vb - va, n);
                        float lambda = -((wallA ? nm_wb : nm_bb) * vn);
                        const float accOld = racc[j];
                        const float newimp = fmaxf(accOld + lambda, 0.0f);
                        lambda = newimp - accOld;
                        racc[j] = newimp;
                        const kb_pair P = pk_splat(lambda) * n;
                        RB_VEL(ra[j]) = pk_store(va - pk_splat(ima) * P);
                        RB_VEL(rb[j]) = pk_store(vb + pk_splat(imb) * P);
                    }
                    wave_sync();
                }
            }
        }
        KB_STAMP_PRE(30);    // ... + its 10 velocity sweeps
    }
    // From here to the end of the position sweeps a wave runs through in its own instruction stream (wave_sync() only): it
    // touches nothing but the bodies of its own islands, so the env no longer pays the slowest wave of the velocity sweeps, then
    // the integration, then the slowest wave of the position sweeps -- which are usually different waves -- but the slowest
    // wave of both together.  What made the two workgroup barriers necessary was the integration by the thread that owns a
    // kilobot by id; a kilobot with a swept contact is now integrated by the lane that holds its LAST contact in canonical
    // order (the one whose depth is bodyDepth[x] after the depth pass; a wall contact names its kilobot once), every other one
    // (no contact, or contacts of a sleeping island only) by its owner thread, which learns it from one bit per slot that the
    // grouping pass left in intMark in front of the set-up barrier.  The owner thread keeps the angle in either case.
    KB_STAMP(4);           // (profile build) wave 0: warm start and its ten sweeps done -- wave-local
    KB_RETID();
    KB_ABLATE_EXIT(11);    // velocity sweeps
    // StoreImpulses: the contact is staged at its position in the packed list, which goes out as a whole at the end of the substep
    if (solving) {
#pragma unroll
        for (int j = 0; j < KRB; ++j)
            if (lane + 64u * j < mycnt) lAcc[RB_C(j)] = racc[j];
    }
    // integrate positions (b2Island::Solve)
    {
        // (islWave is idle from here on) island state for the sleep bookkeeping: bit 1 = has an awake body,
        // bit 0 = position constraints not solved (set by the last position sweep; always without sweeps)
        const unsigned char unsolved = (unsigned char)(posIters <= 0 ? 1 : 0);
        char *const sxB = reinterpret_cast<char *>(startX), *const syB = reinterpret_cast<char *>(startY);
        // one body: the pose at the start of the substep (continuous step), the clamped velocity and the new position;
        // off8 = byte offset of the body inside the float2 arrays
        auto integrate_xy = [&](const unsigned off8, const float2 v0, const float2 p0) __attribute__((always_inline)) {
            kb_pair v = pk_load(v0);
            *reinterpret_cast<float *>(sxB + (off8 >> 1)) = p0.x; *reinterpret_cast<float *>(syB + (off8 >> 1)) = p0.y;
            const kb_pair t = pk_splat(h) * v;
            const float tt = pk_dot(t, t);
            if (tt > B2_MAX_TRANSLATION_SQ) {
                const float ratio = B2_MAX_TRANSLATION / sqrtf(tt);
                v = v * pk_splat(ratio);
            }
            RB_POS(off8) = pk_store(pk_load(p0) + pk_splat(h) * v);
            RB_VEL(off8) = pk_store(v);
        };
        // Who integrates: the depths of both bodies of both slots and the owner thread's marker bits are read before anything
        // is written -- startY lies over bodyDepth, and a lane may look at a body whose last contact another lane holds.
        // Then one trip per register slot, with the owner thread's kilobot of the same place beside it: what a lane reads
        // and uses there is a body that nobody else writes.
        bool intA[KRB], intB[KRB], own[BPT];
        {
            unsigned dA[KRB], dB[KRB], mk[BPT];
            const char *const bdB = reinterpret_cast<const char *>(islCnt);     // bodyDepth
#pragma unroll
            for (int j = 0; j < KRB; ++j) {
                dA[j] = *reinterpret_cast<const unsigned *>(bdB + ((RB_WALL(j) ? rb[j] : ra[j]) >> 1));
                dB[j] = *reinterpret_cast<const unsigned *>(bdB + (rb[j] >> 1));
            }
#pragma unroll
            for (int q = 0; q < BPT; ++q) mk[q] = intMark[(unsigned)ms[q] & 31u];
#pragma unroll
            for (int j = 0; j < KRB; ++j) {
                const unsigned d = (unsigned)RB_DEPTH(j);       // (0: no contact, or one of a sleeping island -- in no round)
                intA[j] = solving && d != 0u && !RB_WALL(j) && dA[j] == d;
                intB[j] = solving && d != 0u && dB[j] == d;
            }
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                own[q] = tid + q * nt < N && ((mk[q] >> ((unsigned)ms[q] >> 5)) & 1u) == 0u;
            }
        }
        wave_sync();
        static_assert(KRB == BPT, "a register slot and a kilobot of the owner thread share a trip");
#pragma unroll
        for (int j = 0; j < KRB; ++j) {
            const unsigned oo = 8u * (unsigned)ms[j];
            const float2 vO = RB_VEL(oo), pO = RB_POS(oo);
            const unsigned char aO = SLEEP ? active[ms[j]] : (unsigned char)1;
            if (j == 0 || mycnt > 64u) {        // (wave-uniform: most waves hold nothing in the slots behind slot 0)
                const float2 vA = RB_VEL(ra[j]), vB = RB_VEL(rb[j]), pA = RB_POS(ra[j]), pB = RB_POS(rb[j]);
                if (intA[j]) {
                    integrate_xy(ra[j], vA, pA);
                    // (the island is awake; only the root's entry is ever read)
                    if (SLEEP) islWave[ra[j] >> 3] = (unsigned char)(2 | unsolved);
                }
                if (intB[j]) {
                    integrate_xy(rb[j], vB, pB);
                    if (SLEEP) islWave[rb[j] >> 3] = (unsigned char)(2 | unsolved);
                }
            }
            if (own[j]) {
                integrate_xy(oo, vO, pO);
                if (SLEEP) islWave[ms[j]] = (unsigned char)((aO ? 2 : 0) | unsolved);
            }
            // the angle never leaves the registers of the owner thread (a thread without a kilobot in this place turns a zero
            // that nobody stores)
            float ww = bw[j];
            const float rot = h * ww;
            if (rot * rot > B2_MAX_ROTATION_SQ) {
                const float ratio = B2_MAX_ROTATION / fabsf(rot);
                ww *= ratio;
            }
            th[j] += h * ww;
            bw[j] = ww;
        }
    }
    wave_sync();
    KB_STAMP(5);           // (profile build) ... + impulses stored, its kilobots integrated -- wave-local
    KB_ABLATE_EXIT(12);    // impulses stored, positions integrated
    // SolvePositionConstraints; an island stops once its minSeparation >= -3 slop.  The island flags are read once per
    // iteration; depth levels without an active contact in this wave are skipped altogether.
    // (The round stays component by component: on pairs it issued fewer instructions and took wave 0 5 % longer -- its
    //  chain runs through the refinements of kb_exact.h, and a packed result costs the instruction behind it a wait state --
    //  and the launch 0.3 % more: profiles/r14_ab_bench.txt.)
    if (solving) {
        for (int it = 0; it < posIters; ++it) {
            unsigned char *act = active + (it & 1) * NB, *nxt = active + ((it + 1) & 1) * NB;
            bool viol = false;
            bool ron[KRB];
#pragma unroll
            for (int j = 0; j < KRB; ++j) ron[j] = (lane + 64u * j < mycnt) && act[RB_ISL(j)] != 0;
#pragma unroll
            for (int j = 0; j < KRB; ++j) {
                for (int d_ = dlo[j]; d_ <= dhi[j]; ++d_) {
                    if (ron[j] && RB_ON(j)) {
                    const bool wallA = RB_WALL(j);
                    const int isl = RB_ISL(j);
                    float nx, ny, sep;
                    const float ima = wallA ? 0.0f : ca.im_bot, imb = ca.im_bot;
                    const float2 pb = RB_POS(rb[j]);
                    const float bx = pb.x, by = pb.y;
                    float axx = 0.0f, ayy = 0.0f;
                    if (wallA) {
                        float dist, wx, wy;
                        wall_geom(ca, RB_WALLIDX(j), bx, by, dist, wx, wy);
                        nx = RB_FLIP(j) ? -wx : wx; ny = RB_FLIP(j) ? -wy : wy;   // manifold normal fixed at detection
                        const float along = RB_FLIP(j) ? -dist : dist;
                        sep = along - B2_POLYGON_RADIUS - ca.r_bot;
                    } else {
                        const float2 pa = RB_POS(ra[j]);
                        axx = pa.x; ayy = pa.y;
                        const float dx = bx - axx, dy = by - ayy;
                        const float dd = dx * dx + dy * dy;
                        // The round is a chain of dependent instructions, and most of them were the IEEE sequences of sqrtf and
                        // the division.  With every pair of the round inside the proven range (wave-uniform test; it also
                        // rules out len < B2_EPSILON) one correction step on the hardware seeds gives the same bits (kb_exact.h).
                        if (__builtin_expect(__builtin_amdgcn_ballot_w64(!kb_exact_guard(dd)) == 0ull, 1)) {
                            const float len = kb_sqrt_refine(dd, __builtin_amdgcn_sqrtf(dd), __builtin_amdgcn_rsqf(dd));
                            const float inv = kb_rcp_refine(len, __builtin_amdgcn_rcpf(len));
                            nx = dx * inv; ny = dy * inv;
                        } else {
                            const float len = sqrtf(dd);
                            nx = dx; ny = dy;
                            if (!(len < B2_EPSILON)) { const float inv = 1.0f / len; nx = dx * inv; ny = dy * inv; }
                        }
                        sep = (dx * nx + dy * ny) - ca.r_bot - ca.r_bot;
                    }
                    if (sep < -3.0f * B2_LINEAR_SLOP) { nxt[isl] = 1; viol = true; if (SLEEP && it == posIters - 1) islWave[isl] = 3; }
                    const float C = kb_clampf(B2_BAUMGARTE * (sep + B2_LINEAR_SLOP), -B2_MAX_LINEAR_CORRECTION, 0.0f);
                    const float K = ima + imb;
                    const float imp = __builtin_expect(ca.exact_div, 1) ? kb_div_const(-C, K, wallA ? ca.y_wb : ca.y_bb) : (K > 0.0f ? -C / K : 0.0f);
                    const float Px = imp * nx, Py = imp * ny;
                    if (!wallA) RB_POS(ra[j]) = make_float2(axx - ima * Px, ayy - ima * Py);
                    RB_POS(rb[j]) = make_float2(bx + imb * Px, by + imb * Py);
                    }
                    wave_sync();
                }
            }
#ifdef KB_PROFILE
            if (tid == 0) atomicAdd(&KB_PROF(10), 1u);
#endif
            if (!__any(viol)) break;
            // the flags the next sweep sets must start cleared (only this wave's islands)
#pragma unroll
            for (int j = 0; j < KRB; ++j) if (lane + 64u * j < mycnt) act[RB_ISL(j)] = 0;
            wave_sync();
        }
        KB_STAMP_PRE(24);    // (profile build) wave 0's own position sweeps, before it waits for the slowest wave
    }
#ifdef KB_SOLVER_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
#undef RB_WALL
#undef RB_WALLIDX
#undef RB_VEL
#undef RB_POS
#undef RB_C
#undef RB_DEPTH
#undef RB_FLIP
#undef RB_ISL
#undef RB_ON
}
