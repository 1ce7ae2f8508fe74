// The loop of the persistent path kernels, included as the body of both kernel
// templates in path_kernels.h (path_kernel_persistent, path_kernel_persistent_blocks)
// so that each compiles exactly as if it were written out.  The including kernel
// provides: template parameters STATS, SINGLE, WIDE, FULL; the type OWN (ownership
// policy, common.h); its arguments S_arg, P_arg, s1, s2, items, cursor, counters,
// PS, tbl; and own_tbl (OwnList's tables, never read under OwnModulo).
    // Work item k renders pass slot k / PS.per_pass (sampler tables at
    // s1/s2 + slot * tbl) of work item k % PS.per_pass; every finished sample
    // goes to its own slot, folded into the framebuffer afterwards (store_sample).
    // The scene and pass records are read in place from the kernel-argument
    // segment (scalar loads at their uses) rather than held in SGPRs for the
    // kernel's lifetime: 100+ live SGPRs spilled into VGPR lanes and from
    // there to scratch.  C3 3184 -> 3310, C5 1662 -> 1772 Mrays/s; VGPR spills
    // lean 10 -> 0, full 98 -> 40 (profiles/r03_park_slack_ab.txt).
    const DevScene& S = kernarg_ref<DevScene>(S_arg, 0);
    const PathParams& P = kernarg_ref<PathParams>(P_arg, kernarg_next<DevScene, PathParams>(0));
    // OwnList: the item -> pixel map goes through tables, so it is evaluated once, at
    // the refill: the sample's landing code (all store_sample needs of the pixel) rides
    // in the top bits of the parked work item word (items < 2^kListItemBits, host).
    constexpr bool kList = std::is_same<OWN, OwnList>::value;
    // tail hand-over (traverse.h CTL_TAIL_LANES): the SINGLE kernels without statistics
    constexpr bool kTail = SINGLE && !STATS && CTL_TAIL_LANES > 0;
    CTL_LANE_STACK_REC(st, kTail ? kTailRecWords + 1 : 0);   // the record and the kept stack pointer
    SamplerDev rng{s1, s2, P.nseq, P.len, 0, 0, 0, 0};
    // work item of the lane's path (pass slot * PS.per_pass + item), parked in
    // LDS for the path's lifetime instead of holding a VGPR through the traces
    int* pkw = ctl_lds_stack + kPathWordOff + threadIdx.x;
    const Park park{(int)threadIdx.x};
    auto split = [&](uint32_t k, uint32_t& ps, uint32_t& kk) { PS.split(k, ps, kk); };
    PathVars v;
    ShadowReq sh;
    sh.valid = false;
    sh.dist = 0.0f;
    TraceStats ts{0, 0, 0};
    uint32_t rays = 0;
    bool active = false, exhausted = false, shadowPhase = false, ending = false, ok = true;
    // kTail: the lane's pending ray is part-way through its traversal (record above its stack top)
    bool susp = false;
#ifdef CTL_PROFILE_TRACE
    long long prof_trace = 0;
    const long long prof_start = wall_clock64();
#endif
    const bool shadowAny = P.shadow_any_hit != 0;
    while (true) {
        const bool need = !active && !exhausted;
        const uint64_t mask = __ballot(need);
        if (mask) {
            const uint64_t k64 = wave_claim(cursor, mask);
            if (need) {
                if (k64 >= items) {
                    exhausted = true;
                } else {
                    const uint32_t k = (uint32_t)k64;   // items < 2^32 (checked on the host)
                    uint32_t px, py, ps, kk;
                    split(k, ps, kk);
                    // FULL: the pass record read through an opaque pointer here, so the
                    // divisions by its fields keep their reciprocals local to the refill
                    // (hoisted, they held VGPRs the FULL kernel spilled for its lifetime;
                    // the lean kernel has the registers and keeps them hoisted)
                    const PathParams& Pw = FULL ? *opaque_ptr(&P) : P;
                    const uint32_t* const T = own_tbl;
                    if (OWN::work_pixel(Pw, T, kk, px, py)) {
                        const uint32_t idx = py * Pw.width + px;
                        // the pass slot's tables start ps * tbl elements in: folded into
                        // the two sequence offsets so the table bases stay kernel-uniform
                        rng.a = idx % Pw.nseq + ps * tbl; rng.b = (idx / Pw.nseq) % Pw.nseq + ps * tbl;
                        rng.d1 = 0; rng.d2 = 0;
                        if constexpr (!kList) *pkw = (int)k;
                        f3 o, dw;
                        const f2 pX = primary_ray<FULL>(S, rng, px, py, o, dw);
                        if constexpr (kList) *pkw = (int)(k | landing_code(Pw, px, py, pX) << kListItemBits);
                        v.begin(pX, o, dw);
                        shadowPhase = false;
                        ending = false;
                        // loop head of PathTrace: `while (depth++ < MaxPathLength)`
                        if (!OWN::apron_keep(Pw, T, kk, pX)) PS.s[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        else if (v.depth++ < P.max_path_length) active = true;
                        else store_sample(P, PS, ps, kk, px, py, v.pX, mk3s(1.0f) * v.cl);
                        if (active) park.begin(v, rng);
                    } else {
                        PS.s[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // work item outside the image: no sample
                    }
                }
            }
        }
        if (!__any(active)) {
            if (__all(exhausted)) break;
            continue;
        }
        if (active) {
            HitRec h = no_hit((shadowPhase && shadowAny) ? sh.dist - S.ray_eps : FLT_MAX);
            if (!kTail || !susp) rays++;   // a handed-over ray was counted at its first call
#ifdef CTL_PROFILE_TRACE
            const long long pc0 = wall_clock64();
#endif
            if (S.n_nodes != 0) {
                Traverser<2, STATS, SINGLE, WIDE, CTL_ALPHA_OF(FULL)> T;
                T.anyhit = shadowPhase && shadowAny;
                // a handed-over lane sets up the same ray by the same calls on the same
                // inputs (the sentinel init pushes is the one already at the bottom; init
                // also clears the overflow flag, which is why `ok` takes it after every call)
                T.init(S, v.rori, shadowPhase ? sh.d : v.rdir, 0.0f, S.ray_eps, h.t, st, &ts,
                       T.anyhit ? sh.dist : -1.0f);
                if constexpr (kTail) {
                    // ... then takes back its stack top and its record
                    if (susp) { st.sp = st.kept_sp(); T.resume(st); }
                    // Break rule.  `entered` lanes run this call; the lanes still in the
                    // loop after a round vote (the ballot sees exactly them, so the
                    // outcome is uniform among them and they leave together): hand over
                    // once fewer than CTL_TAIL_LANES per 64 entered lanes still traverse.
                    // Relative to `entered`, so the few lanes of a wave at the end of a
                    // launch (entered * CTL_TAIL_LANES <= 64) are never cut.
                    // Progress: (1) every call runs at least one round for every
                    // unfinished lane before the first vote; (2) in >= 1, CTL_TAIL_LANES
                    // < 64, so in * 64 < entered * CTL_TAIL_LANES implies in < entered: a
                    // break happens only when a ray of this call has finished; (3) so
                    // every iteration of the persistent loop finishes a ray or advances
                    // every open traversal by a round, and a traversal is a finite
                    // number of rounds: the loop ends as the loop without the rule does.
                    const uint32_t entered = (uint32_t)__popcll(__ballot(1));
                    for (;;) {
                        T.round(S, st, &ts);
                        if (T.done) break;
                        const uint64_t inm = __ballot(1);
                        const uint32_t in = (uint32_t)__popcll(inm);
                        if (in * 64u < entered * (uint32_t)CTL_TAIL_LANES) {
                            // counted here, one atomic pair per break: counts carried in
                            // registers through the loop cost the FULL kernel 13 -> 38 spilled VGPRs
                            if ((int)(threadIdx.x & 63) == __ffsll((unsigned long long)inm) - 1) {
                                atomicAdd(&counters[kTailHandovers], (unsigned long long)in);
                                atomicAdd(&counters[kTailBreaks], 1ull);
                            }
                            break;
                        }
                    }
                    susp = !T.done;
                    // sp goes to a private word of its own: nothing of the stack is live in shading
                    if (susp) { T.suspend(st); st.keep_sp(); }
                    else h = T.h;
                } else {
                    while (!T.done) T.round(S, st, &ts);
                    h = T.h;
                }
                ok &= !st.overflow;
            }
#ifdef CTL_PROFILE_TRACE
            prof_trace += wall_clock64() - pc0;
#endif
            // a suspended lane skips all of the shading: its path state stays parked, its
            // pending ray in the registers that hold it (v.rori, v.rdir / sh.d, sh.dist, shadowPhase)
            if (!kTail || !susp) {
                // the FULL kernels read parked state where the shading uses it (Park's
                // partial loads), the lean kernel all of it after the trace
                constexpr bool lazy = FULL != kShadeLean;
                if (lazy) park.load_core(v, rng);
                else park.load(v, sh, rng);
                bool cont;
                // kShadeMedia: the medium step in front of the split into miss and hit (shading.h
                // medium_step); `scattered`: it took the iteration, no surface is shaded
                constexpr bool kMedia = CTL_MEDIA_OF(FULL);
                bool scattered = false;
                if constexpr (kMedia) {
                    if (!shadowPhase) {
                        park.load(v, sh, rng);
                        const int ev = medium_step<FULL>(S, P, rng, v, h, sh);
                        if (ev != kMediumNone) {
                            scattered = true;
                            v.vol_miss = h.tri == 0xffffffffu;
                            ending = ev == kMediumEnded;
                            shadowPhase = sh.valid;
                            cont = sh.valid || (!ending && v.depth++ < P.max_path_length);
                            // the loop ends with r2 still a miss: PathTracer.cu:98-111 along the new ray
                            if (!cont && v.vol_miss) v.cl = v.cl + env_miss<FULL>(S, P, v);
                        }
                        // cf (a hit behind the medium) and the sampler's position go back to the park
                        if (!scattered || cont) park.store_shaded(v, sh, rng);
                    }
                }
                if (scattered) {
                } else if (shadowPhase) {
                    if (lazy) { v.cl = park.get3(0); sh.add = park.get3(16); }
                    if (!shadow_occluded(S, shadowAny, h, sh.dist)) v.cl = v.cl + sh.add;
                    shadowPhase = false;
                    cont = !ending && v.depth++ < P.max_path_length;
                    if constexpr (kMedia) {
                        if (!cont && v.vol_miss) {   // as above, after the light sample's term
                            const spec cl = v.cl;
                            const int depth = v.depth;
                            park.load(v, sh, rng);
                            v.depth = depth;
                            v.cl = cl + env_miss<FULL>(S, P, v);
                        }
                    }
                    if (lazy && cont) { park.store_cl(v); park.store_depth(v); }
                } else if (h.tri == 0xffffffffu) {
                    if (lazy) park.load(v, sh, rng);
                    v.cl = v.cl + env_miss<FULL>(S, P, v);   // PathTracer.cu:98-111
                    cont = false;
                } else {
                    // the FULL kernel keeps the path's first-hit texture partials in its own
                    // sample slot (written only when the path ends), not in four VGPRs
                    // carried through every trace
                    float4* part = kList ? PS.s + ((uint32_t)*pkw & kListItemMask) : PS.s + *pkw;
                    if constexpr (kMedia) v.vol_miss = false;
                    ending = lazy ? !shade_hit<FULL, SINGLE, Park>(S, P, rng, v, h, sh, part, &park)
                                  : !shade_hit<FULL, SINGLE>(S, P, rng, v, h, sh, part);
                    shadowPhase = sh.valid;
                    cont = sh.valid || (!ending && v.depth++ < P.max_path_length);
                    if (lazy && cont) park.store_shaded(v, sh, rng);
                }
                if (!cont) {
                    if constexpr (kList) {
                        const uint32_t wd = (uint32_t)*pkw;   // one pass per launch: the item is the slot
                        store_sample_coded(PS, wd & kListItemMask, wd >> kListItemBits, mk3s(1.0f) * v.cl);
                    } else {
                        uint32_t px, py, ps, kk;
                        split((uint32_t)*pkw, ps, kk);
                        const PathParams& Pw = FULL ? *opaque_ptr(&P) : P;   // as at the refill
                        OWN::work_pixel(Pw, own_tbl, kk, px, py);
                        if (lazy) park.load_px(v);
                        store_sample(Pw, PS, ps, kk, px, py, v.pX, mk3s(1.0f) * v.cl);
                    }
                    active = false;
                } else if (!lazy) {
                    park.store(v, sh, rng);
                }
            }
        }
    }
    wave_add_u64(&counters[0], rays);
    flush_counters<STATS>(counters, !ok, ts);
#ifdef CTL_PROFILE_TRACE
    // wall-clock ticks (100 MHz) per wave: in the trace call site / in the kernel
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&counters[5], (unsigned long long)prof_trace);
        atomicAdd(&counters[6], (unsigned long long)(wall_clock64() - prof_start));
    }
    wave_add_u64(&counters[8], ts.inner_lanes);
    wave_add_u64(&counters[9], ts.inner_waves);
    wave_add_u64(&counters[10], ts.leaf_lanes);
    wave_add_u64(&counters[11], ts.leaf_waves);
    wave_add_u64(&counters[12], ts.inner_r);
    wave_add_u64(&counters[13], ts.rounds);
    wave_add_u64(&counters[14], ts.leafphase_in);
#endif
