// mgx_fused_body.inc -- the body of the fused kernel (mgx_fused.h), included textually by its entry points so that each is compiled
// exactly as if the body were written in it.  It expects these names in scope, as compile-time constants, and `a` (KernelArgs):
//     V, MODE, HOOKS, AR, OH, GEN, STREAM, DMA, GRP, SHAPE, C8, B3
// mgx_fused_kernel takes all twelve as its template parameters, in this order; mgx_obs_kernel (= MODE 0 with an occupancy request),
// mgx_resident_kernel (= kShapes 9 with one) and the runtime-compiled shape kernels (multigrid_amd/jit.py: source_for) take some and
// define the rest, in this order too.
    constexpr bool DO_STEP = MODE != 0;
    const int env_kind = HOOKS ? a.sp.env_kind : (int)MGX_KIND_EMPTY;
    constexpr bool PERSIST = MODE == 3;         // persistent stepping: the rollout's step loop, each step's actions handed over as
                                                // tagged granules, a per-wavefront flag published behind its outputs (include/mgx.h)
    constexpr bool ROLL = MODE == 2 || PERSIST;
    // cache policy of everything a step hands to its consumer: the persistent kernel never ends between steps, so there is no
    // end-of-kernel write-back to make its stores visible -- they are written THROUGH to memory (sc1, aux 16) and the flag
    // follows an s_waitcnt vmcnt(0) (guide: publish/consume recipe R1)
    constexpr int kOutAux = PERSIST ? 16 : kSmallOutAux;
    // (base: wave-uniform pointer to the wavefront's first element, idx: this lane's element, n: elements of the wavefront)
#define MGX_PUB_STORE_U8(base, idx, n, val)                                                                            \
    do {                                                                                                               \
        if constexpr (PERSIST) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(val), make_rsrc((base), (n)), (idx), 0, 16); \
        else (base)[idx] = (uint8_t)(val);                                                                           \
    } while (0)
    // MARK: the one-step kernels with the fused auto-reset keep the per-env layout marker of mgx_step_tracked (include/mgx.h,
    // KernelArgs::grid_layout) when the launch has one: a restart stores the layout's index, a cell written back to the grid stores
    // -1.  MARK_RD: the throughput family also READS it in P0 where the host asks for it (a.flags bit 2) -- a runtime, wave-uniform
    // branch inside the existing instantiations, none of its own
    constexpr bool MARK = AR && MODE == 1 && !GEN && !C8 && !B3;
    constexpr bool MARK_RD = MARK && !DMA;
    constexpr int V2 = V * V;
    constexpr int NW = (V2 + 63) / 64;          // 64-bit mask words per view = lane passes per view
    constexpr int CB = C8 ? 1 : kCellBytes;      // bytes per grid cell: MgxCell, or the compact MgxCell8 (include/mgx.h)
    // (round 6: + the step with ONE-HOT output -- what RLlib's default registration feeds the policy, multigrid/rllib/__init__.py:
    // 110-111: the decode table's entries are then the cells' one-hot MASKS, so P4' is a select and a store per cell)
    // (... and the hook-free rollout / persistent kernels: a 64x64 env's tile is 4 KiB there)
    static_assert(!C8 || (!GEN && !DMA && (MODE < 2 ? (!OH || (MODE == 1 && !HOOKS)) : (!OH && !HOOKS))),
                  "compact cells: the plain step / gen_obs kernels, the step with one-hot output, the hook-free rollout / persistent kernels");
    static_assert(SHAPE == 0 || kShapes[SHAPE].cb == CB, "shape table entry of the other cell format");
    // B3: the grid tensors in HBM (grid, pool_grid) are the REFERENCE's byte triples u8[B,H,W,3] (MgxSpec.cell_bytes = 3): P0 packs
    // them into the 16-bit LDS tile as they arrive, the dirty cells go back as three bytes -- a caller that holds the north star's
    // (B,H,W,3) uint8 tensor pays the conversion inside the step's own launch instead of two extra launches around it
    static_assert(!B3 || (!C8 && !OH && !GEN && !DMA && MODE < 2 && SHAPE == 0), "byte grids: the plain step / gen_obs kernels only");
    constexpr int CBG = B3 ? 3 : CB;             // bytes per cell of the grid tensors in HBM
    // RSHAPE: a RESIDENT shape of the rollout / persistent kernels (mgx_fused.h: kShapes[].ns > 0; round 6): 64 view slots with two
    // slots per cell register like the throughput step kernel, and NS slices of Gw envs per wavefront, stepped one after the other
    // (LdsCarve: what lives across steps once per slice, the per-step temporaries once per wavefront)
    constexpr bool RSHAPE = SHAPE != 0 && kShapes[SHAPE].ns > 0;
    constexpr int NS = RSHAPE ? kShapes[SHAPE].ns : 1;
    // PITCH: the tile's row pitch when rows and envs share the WALL ring (kShapes 9: 15 for the 16x16 grid), 0 = the grid's own width;
    // SLICED: the LDS layout of the sliced kernels (per-step temporaries once per wavefront, staging over the view records)
    constexpr int PITCH = RSHAPE ? kShapes[SHAPE].pitch : 0;
    constexpr bool SLICED = RSHAPE && shape_sliced(kShapes[SHAPE]);
    static_assert(!RSHAPE || ((MODE == 2 || MODE == 3) && !OH && !GEN && !STREAM && !DMA && !C8 && !B3 && V <= 7), "resident shapes: rollout / persistent kernels");
    static_assert(NS <= 2, "slices: the (step, slice) sequence below is written for one or two");
    constexpr bool HALF = !DMA && (MODE == 1 || RSHAPE) && !C8;   // cell registers hold two slots' packed cells each (throughput step kernels)
    constexpr bool PK3 = kPack3<V>;              // 9x9 views: three views' 17-cell remainders share a lane pass (mgx_fused.h)
    // LINES: P2 / P4 with one lane per view LINE instead of one per cell (mgx_fused.h gather_lines): the kernels of the dword staging
    // on 16-bit tiles -- the same compile-time condition, no instantiation of its own
    constexpr bool LINES = view_line_lanes(V, ROLL, OH, C8, GRP);
    // GRP: view slots gathered (P2) / written (P4) as one straight-line block and staged per P4/P5 round.  16 everywhere but in
    // the small-group latency instantiations (DMA, GRP 4 or 8), whose wavefronts own exactly ONE group: a wave of 4 views runs 4
    // slots of P2/P4/P5, not 16 -- on a lone wave's instruction chain that is the difference (plan_launch picks them)
    constexpr int kG = GRP, kR = SLICED ? kRoundResident : GRP;   // (sliced kernels: the staging of a round lies over the view records: 8 slots)
    constexpr int kG4 = kR < kG ? kR : kG;                          // P4's straight-line blocks: within one round
    constexpr int VPW = (DMA && GRP < kGroup) ? GRP : ((V <= 7 && HALF) ? kSlotsSmallView : 32);   // view slots per wavefront
    extern __shared__ __align__(16) uint8_t lds[];

    int lane_ = threadIdx.x & 63;
#define lane lane_

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // The kernel arguments P0's load burst needs, fetched in ONE batch of scalar loads at the wavefront's first instructions: left to
    // the compiler they came in four dependent s_load / s_waitcnt pairs, each a scalar-memory round trip in front of the tile burst
    // Every instantiation with views <= 7x7: first the latency family only (a lone wavefront's instruction chain), then the C4
    // throughput kernel too (18.63-18.83 -> 18.45-18.54 us, three same-box passes); 9x9 and up: the compiler crashes on it.
    if constexpr (V <= 7) {
        const int64_t e_batch = a.batch;
        const uint8_t *e_grid = a.grid, *e_agents = a.agents, *e_aux = a.aux, *e_hord = a.hook_order;
        const uint64_t *e_rng = a.rng;
        const int32_t *e_sc = a.step_count;
        const int8_t *e_act = a.actions;
        const unsigned e_bd = blockDim.x;
        const int32_t *e_ep = (AR || GEN) ? a.episode : nullptr;
        const uint8_t *e_trunc = DO_STEP ? a.truncated : nullptr;      // (its kernarg line holds the output pointers MGX_LATE asks for later)
        const uint64_t *e_gs = GEN ? a.gen.gen_state : nullptr;       // (GEN: the generator's and the staging slots' lines)
        const int32_t *e_tag = GEN ? a.gen.stage.tag : nullptr;
        const int32_t *e_lay = MARK_RD ? a.grid_layout : nullptr;     // (MARK_RD: the marker and the pool, for P0's first load)
        const uint8_t *e_pool = MARK_RD ? a.pool_grid : nullptr;
        asm volatile("" :: "s"(e_batch), "s"(e_grid), "s"(e_agents), "s"(e_rng), "s"(e_sc), "s"(e_act), "s"(e_hord), "s"(e_aux),
                     "s"(e_bd), "s"(e_ep), "s"(e_trunc), "s"(e_gs), "s"(e_tag), "s"(e_lay), "s"(e_pool));
    }
    // SHAPE != 0: an instantiation for ONE (W, H, A, envs per wavefront) of mgx_fused.h's kShapes -- the latency family's answer to
    // what a lone wavefront pays for a runtime shape: every LDS offset of the carve, the agent loops, the row pitch and the
    // lane -> (env, agent) split become immediates (C2: a wave lives 3.78 instead of 4.24 us, BlockedUnlockPickup at 16384
    // envs 4.45 instead of 5.08; round 3).  The launcher picks it only when the launch geometry matches exactly (choose_in_family).
    constexpr bool FIXED = SHAPE != 0;
    // Two rare-path refinements for big envs (many agents: the shortened sequential fallback; layouts of >= 4 KiB: the vectorised
    // restart copy) are compiled into the one-step kernels for views of 9x9 and more (and the C5 shape) only -- big views are what big
    // envs use --: the instantiations for small views -- the C4 headline, the latency family -- and the rollouts keep the simple forms (measured, same box: the general forms cost C4 +1.4 %, C3
    // +0.9 % in registers and code they never run, and gain C5 1.5 %)
    constexpr bool PREFIX = FIXED ? (kShapes[SHAPE].A > 4) : (V > 7 && MODE == 1);
    constexpr bool BIGCOPY = FIXED ? (kShapes[SHAPE].W * kShapes[SHAPE].H * CB >= 4096) : (V > 7 && MODE == 1);
    const int W = FIXED ? kShapes[SHAPE].W : a.sp.width, H = FIXED ? kShapes[SHAPE].H : a.sp.height,
              A = FIXED ? kShapes[SHAPE].A : a.sp.num_agents;
    const int Gw_ = FIXED ? kShapes[SHAPE].Gw : a.Gw;                               // envs per wavefront
    const int vpw_ = FIXED ? shape_slots(kShapes[SHAPE]) : a.vpw;                   // view slots in use
    const int inv_A_ = FIXED ? (65536 + kShapes[SHAPE].A - 1) / (FIXED ? kShapes[SHAPE].A : 1) : a.inv_A;
    const int HWB = H * W * CB;                             // bytes of one env's grid (packed cells)
    const int HWG = H * W * CBG;                            // ... in the HBM tensors (== HWB unless B3)
#define MGX_LATE_GEN(f) kernarg_at<decltype(MgxLayoutGen::f)>(offsetof(KernelArgs, gen) + offsetof(MgxLayoutGen, f))
#define MGX_LATE_STAGE(f) kernarg_at<decltype(MgxGenStage::f)>(offsetof(KernelArgs, gen) + offsetof(MgxLayoutGen, stage) + offsetof(MgxGenStage, f))
    if constexpr (GEN && MODE == 1) {
        // ---------------------------------------------------------------- GENERATOR wavefronts (include/mgx.h: MgxGenStage): the
        // workgroups behind the step's own.  One lane per env: an env whose step took a snapshot in an EARLIER launch (two steps
        // before its truncation) gets its next episode generated into its staging slot -- beside the step, not behind it.
        if ((int64_t)blockIdx.x >= a.gen_first_wg) {
            const int64_t gw = ((int64_t)blockIdx.x - a.gen_first_wg) * (blockDim.x >> 6) + wave;
            const int64_t b = gw * 64 + lane;
            int32_t *const tag = MGX_LATE_STAGE(tag);
            // (MgxGenStage.candidates are made by a kernel of their own: mgx_layout_gen.hip, stage_candidates_kernel)
            const int32_t phase1 = MGX_LATE_STAGE(phase) + 1;
            // the request word is published LAST by the step's wavefront (release) and read FIRST here (acquire): a request that
            // is seen is seen with its snapshot.  A request of an episode the env has left is dropped.
            // (external == 2: this launch runs BETWEEN two steps on their stream -- nothing writes a tag beside it, plain accesses do)
            const bool serial = MGX_LATE_STAGE(external) == 2;
            int32_t req = b >= a.batch ? 0 : serial ? tag[b * 4 + 3]
                                                    : __hip_atomic_load(tag + b * 4 + 3, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (req != 0 && req != phase1 && tag[b * 4 + 1] != a.episode[b]) { tag[b * 4 + 3] = 0; req = 0; }
            const bool go = req != 0 && req != phase1;              // (a request of THIS launch is not complete yet: next time)
            const uint64_t gom = __builtin_amdgcn_ballot_w64(go);
#if MGX_SPANS
            const int64_t wid_g = a.gen_first_wg * (blockDim.x >> 6) + gw;      // (its span record: behind the step's wavefronts)
            const unsigned long long t_g0 = __builtin_amdgcn_s_memrealtime();
            if (gom == 0 && lane == 0 && a.span_base + wid_g < kSpanCap) {
                g_span[2 * (a.span_base + wid_g)] = t_g0;
                g_span[2 * (a.span_base + wid_g) + 1] = __builtin_amdgcn_s_memrealtime() & 0x0fffffffffffffffull;
            }
#endif
            if (gom == 0) return;
            MGX_RARE_PATH_PRIO();                                    // (the slowest wavefronts of the launch: ahead of their SIMD's others)
            MgxLayoutGen gen;                                        // (field by field: a struct copy would live in scratch memory)
            gen.kind = MGX_LATE_GEN(kind); gen.room_size = MGX_LATE_GEN(room_size);
            gen.start_x = MGX_LATE_GEN(start_x); gen.start_y = MGX_LATE_GEN(start_y); gen.start_dir = MGX_LATE_GEN(start_dir);
            gen.max_hallway_keys = MGX_LATE_GEN(max_hallway_keys); gen.max_keys_per_room = MGX_LATE_GEN(max_keys_per_room);
            gen.blank = MGX_LATE_GEN(blank); gen.gen_state = MGX_LATE_GEN(gen_state);
            uint8_t *const st_grid = reinterpret_cast<uint8_t *>(MGX_LATE_STAGE(grid));
            mgx_gen::copy_blank(gen, st_grid, gw * 64, HWB, gom, lane);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (the owning lane overwrites cells the other lanes stored)
            __builtin_amdgcn_s_waitcnt(0x0F70);
            wave_sync();
            if (go) {
                const int32_t ep_s = tag[b * 4 + 1], sc_s = tag[b * 4 + 2];
                uint64_t *const words = MGX_LATE_STAGE(words) + b * 12;
                const uint64_t *gs = gen.gen_state + b * 6, *rg = a.rng + b * 4;
                mgx_gen::NpGen lay, npr;
                for (int k = 0; k < 4; ++k) lay.s[k] = gs[k];
                lay.buf = gs[4]; npr.buf = gs[5];
                // env.np_random at reset time = the snapshot + A draws for every step that was left (base.py:396-399)
                uint64_t s0 = words[10], s1 = words[11];
                const uint64_t i0 = rg[2], i1 = rg[3];
                const uint64_t jA[4] = {kJump.w[A][0], kJump.w[A][1], kJump.w[A][2], kJump.w[A][3]};     // A draws ahead
                if (A > 1 && a.sp.max_steps > sc_s) pcg64_advance(s0, s1, i0, i1, jA, (uint32_t)(a.sp.max_steps - sc_s));
                npr.s[0] = s0; npr.s[1] = s1; npr.s[2] = i0; npr.s[3] = i1;
                uint8_t *apos = lds + wave * a.wave_lds + lane * (2 * A);          // (the host checked wave_lds >= 128 A)
                const uint4 naux = mgx_gen::generate_episode(gen, W, H, A, lay, npr, apos, st_grid + b * HWB,
                                                             reinterpret_cast<uint64_t *>(MGX_LATE_STAGE(agents)) + b * A);
                uint8_t *const st_aux = MGX_LATE_STAGE(aux);
                if (st_aux) reinterpret_cast<uint4 *>(st_aux)[b] = naux;
                for (int k = 0; k < 4; ++k) { words[k] = lay.s[k]; words[6 + k] = npr.s[k]; }
                words[4] = lay.buf; words[5] = npr.buf;
                // a step wavefront of THIS launch may have taken a fresh snapshot of this env meanwhile (an old request that was
                // still unserved): then what was generated belongs to a request that no longer exists -- publish nothing, leave
                // the fresh request for the next launch
                if (serial) {
                    tag[b * 4 + 3] = 0;                                             // served
                    tag[b * 4] = ep_s;                                              // the slot holds ep_s's successor
                } else {
                    const bool same = __hip_atomic_load(tag + b * 4 + 3, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == req
                                      && tag[b * 4 + 1] == ep_s && tag[b * 4 + 2] == sc_s;
                    if (same) {
                        tag[b * 4 + 3] = 0;                                         // served
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                        __hip_atomic_store(tag + b * 4, ep_s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);   // the slot holds ep_s's successor
                    }
                }
            }
#if MGX_SPANS
            if (lane == 0 && a.span_base + wid_g < kSpanCap) {      // (flag 8 << 60: a generator wavefront that generated)
                g_span[2 * (a.span_base + wid_g)] = t_g0;
                g_span[2 * (a.span_base + wid_g) + 1] = (__builtin_amdgcn_s_memrealtime() & 0x0fffffffffffffffull) | (8ull << 60);
            }
#endif
            return;
        }
    }
    const int64_t wid = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    const int64_t e0w = wid * (Gw_ * NS);                    // first env of this wavefront (its slices: e0w + s * Gw_)
    const int64_t e0 = e0w;                                   // ... of its slice 0 (the only one unless NS > 1)
    if (e0 >= a.batch) return;
    [[maybe_unused]] const int ns_act = NS > 1 ? (int)min((int64_t)NS, (a.batch - e0w + Gw_ - 1) / Gw_) : 1;   // slices that hold envs
    const int Gc = (int)min((int64_t)Gw_, a.batch - e0);    // envs of this wavefront
    const int NVc = Gc * A;                                   // its views (<= VPW)
    const int64_t v0 = e0 * A;                                // first (env, agent) row

#if MGX_TIMESTAMPS
    int stamp_i = 0;
    MGX_MARK("start");
#endif
#if MGX_SPANS
    if (!PERSIST && lane == 0 && a.span_base + wid < kSpanCap) g_span[2 * (a.span_base + wid)] = __builtin_amdgcn_s_memrealtime();
    unsigned long long span_flags = 0;      // which rare paths this wavefront took (bits 60.. of its end record): 1 = auto-reset,
                                            // 2 = sequential fallback (P1b/P1c), 4 = success / failure events, 8 = cell writes
#define MGX_SPAN_FLAG(bit, cond) do { if (!GEN && (cond)) span_flags |= (unsigned long long)(bit); } while (0)
#define MGX_SPAN_GFLAG(bit, cond) do { if (cond) span_flags |= (unsigned long long)(bit); } while (0)   // (GEN kernels: their own flags)
#else
#define MGX_SPAN_FLAG(bit, cond) ((void)0)
#define MGX_SPAN_GFLAG(bit, cond) ((void)0)
#endif
#if MGX_DEBUG_KNOBS
    // tools' build: bits 16..23 of the phase mask = a start stagger, in units of 64 cycles per hardware wave slot of the SIMD
    // (HW_ID[3:0]; bit 24: per (slot & 1) instead): do the load bursts of a SIMD's wavefronts have to collide?  (round 3)
    if (a.dbg >> 16) {
        const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);      // HW_REG_HW_ID
        const int k = ((a.dbg >> 24) & 1) ? (int)(hw & 1u) : (int)(hw & 3u);
        for (int i = 0; i < k * ((a.dbg >> 16) & 0xff); ++i) __builtin_amdgcn_s_sleep(1);
    }
    // bits 25 / 26: a standing issue priority by hardware wave slot (slot & 1 / slot & 3) instead of a stagger: does running the
    // SIMD's wavefronts out of phase -- without making anybody wait -- overlap the VALU-heavy and the LDS-heavy phases?
    if (a.dbg & (3 << 25)) {
        const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
        const uint32_t pr = (a.dbg & (1 << 26)) ? (hw & 3u) : ((hw & 1u) * 2u);
        if (pr == 1) __builtin_amdgcn_s_setprio(1); else if (pr == 2) __builtin_amdgcn_s_setprio(2); else if (pr == 3) __builtin_amdgcn_s_setprio(3);
    }
#endif
    const LdsCarve cv = make_carve(W, H, A, V, Gw_, vpw_, ROLL, HOOKS, OH, kR, CB, NS, SLICED, PITCH);
    // bytes between two envs' cells in the TILE (the HBM tensors: HWB)
    const int TSB = PITCH ? PITCH * (H - 1) * CB : HWB;
    const int wave_lds_ = FIXED ? cv.total() : a.wave_lds;                          // (== the host's wave_lds_bytes: match_fixed_shape checks)
    uint8_t *L = lds + wave * wave_lds_;
    uint64_t *rows = reinterpret_cast<uint64_t *>(L + cv.rows());             // [slot] packed agent rows
    ViewRec *rec = reinterpret_cast<ViewRec *>(L + cv.rec());                 // [slot]
    int8_t *acts = reinterpret_cast<int8_t *>(L + cv.act());                  // [slot]
    uint64_t *rngs = reinterpret_cast<uint64_t *>(L + cv.rng());              // [env][4]
    uint64_t *rnd = reinterpret_cast<uint64_t *>(L + cv.rnd());               // [slot] 53-bit draws
    uint8_t *ord = L + cv.ord();                                               // [slot] visiting order per env
    double *rew = reinterpret_cast<double *>(L + cv.rew());                   // [slot]
    int32_t *scnt = reinterpret_cast<int32_t *>(L + cv.scnt());               // [env]
    uint4 *auxl = reinterpret_cast<uint4 *>(L + cv.aux());                    // [env] 16-byte hook state (include/mgx.h)
    uint64_t *jump = reinterpret_cast<uint64_t *>(L + cv.jump());             // [A+1][4]

    // (read as plain kernel arguments, not MGX_LATE: they are fetched with the launch's first scalar loads -- an s_load of their cold
    // kernarg line in the middle of P0 would sit on the wavefront's critical path)
    [[maybe_unused]] int32_t *const stage_tag = (GEN && MODE == 1 && A > 1) ? a.gen.stage.tag : nullptr;
    [[maybe_unused]] const int cand_K = (GEN && MODE == 1 && A > 1 && a.gen.stage.tag) ? a.gen.stage.candidates : 0;   // (0: the snapshot protocol)
    [[maybe_unused]] uint64_t *const gen_state_p = GEN ? a.gen.gen_state : nullptr;

    MGX_MARK("P0");
    // ------------------------------------------------------------------ P0: HBM -> LDS, all loads in flight at once
    const int64_t g0 = e0 * HWB, g1 = g0 + (int64_t)Gc * HWB;       // byte range of these envs in `grid`
    const int64_t gtotal = a.batch * (int64_t)HWB;
    const int64_t ga = B3 ? g0 : (g0 & ~(int64_t)15);               // (B3: the tile is written cell by cell, no skew)
    uint8_t *tile_raw = L + cv.tile();                              // holds global bytes [ga, ...)
    const int tile_skew = (int)(g0 - ga);
    [[maybe_unused]] uint8_t *tile = tile_raw + tile_skew;           // env e's cells at tile + e*HWB
    // Every HBM load of the wavefront is issued here, back to back, into registers; then ONE unconditional
    // s_waitcnt vmcnt(0); then the LDS stores.  (Waiting under the same lane predicates as the loads makes hipcc's
    // waitcnt pass believe loads may still be pending and sprinkle vmcnt(0) -- which on CDNA also waits for every
    // older global STORE -- over the rest of the kernel.)
    constexpr int U = 8;                                                    // 8 KiB of tile per pass
    const uint8_t *gsrc = a.grid + ga;
    const int len = (int)(g1 - ga);
    const int avail = (int)min(gtotal - ga, (int64_t)INT_MAX);               // bytes readable from gsrc
    // (tools' build: bit 0 = no tile traffic at all, bit 10 = half of it -- what a byte-sized cell format could save at most)
    const int grec = MGX_DBG(1) ? 0 : MGX_DBG(1024) ? min((len / 2 + 15) & ~15, avail) : min((len + 15) & ~15, avail);
    const __amdgpu_buffer_rsrc_t grsrc = make_rsrc(gsrc, grec);
    const int lane16 = 16 * lane;
    const int env_of_lane = (lane * inv_A_) >> 16, agent_of_lane = lane - env_of_lane * A;   // slot `lane` = (env, agent)
    // (0) MARK_RD launches that read the layout marker (a.flags bit 2): env `lane`'s marker goes out FIRST, so that it can be waited
    // for alone -- vmcnt counts in order -- while the small inputs below stay in flight across the branch it decides
    [[maybe_unused]] const bool read_marker = MARK_RD && (a.flags & 4) != 0;                    // wave-uniform
    [[maybe_unused]] int32_t in_lay = -1;
    if constexpr (MARK_RD) {
        if (read_marker) in_lay = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(make_rsrc(a.grid_layout + e0, Gc * 4), lane * 4, 0, 0);
    }
    // (1) what the draws (P1a) need goes out first: this lane's env's PCG64 words and its agent's jump-ahead constants
    u32x4 in_rngA = {0, 0, 0, 0}, in_rngB = {0, 0, 0, 0};                    // (ROLL: two envs' halves, copied to LDS)
    u32x4 in_jmpA = {0, 0, 0, 0}, in_jmpB = {0, 0, 0, 0};
    // (MARK_RD kernels issue these loads whatever A is -- for one agent through a descriptor of no bytes --: the wait for the marker
    // then counts them exactly and leaves them in flight, and a launch that does not read the marker waits for nothing; under a
    // runtime condition the wait-count pass makes every launch wait for them in front of the tile burst)
    if (MARK_RD || (DO_STEP && A > 1)) {
        const __amdgpu_buffer_rsrc_t rr = make_rsrc(a.rng + e0 * 4, (MARK_RD && A <= 1) ? 0 : Gc * 32);
        if (ROLL) {                                                              // env-major copy: lane l holds words 2l, 2l+1
            in_rngA = __builtin_amdgcn_raw_buffer_load_b128(rr, lane16, 0,kInAux);
            for (int t = lane; t < A * 4; t += 64) jump[t] = kJump.w[1][t];          // constants for k = 1..A, re-read every step
        } else {                                                                 // same address for the A lanes of an env
            in_rngA = __builtin_amdgcn_raw_buffer_load_b128(rr, env_of_lane * 32, 0,kInAux);
            in_rngB = __builtin_amdgcn_raw_buffer_load_b128(rr, env_of_lane * 32 + 16, 0,kInAux);
            const u32x4 *jk = reinterpret_cast<const u32x4 *>(&kJump.w[1 + agent_of_lane][0]);   // agent k draws k+1 ahead
            in_jmpA = jk[0]; in_jmpB = jk[1];
        }
    }
    u32x2 in_row = {0, 0};
    uint32_t in_scnt = 0;
    u32x4 in_aux = {0, 0, 0, 0};
    uint8_t in_act = 0;
    [[maybe_unused]] uint8_t in_hord = 0;
    in_row = __builtin_amdgcn_raw_buffer_load_b64(make_rsrc(a.agents + v0 * 8, NVc * 8), lane * 8, 0,kInAux);
    uint32_t in_ep = 0;                                                      // AR / GEN: env `lane`'s episode count
    [[maybe_unused]] int32_t in_tag = -1, in_tag_sc = -1;                   // GEN with staging: tag[0] (slot's episode), tag[2] (its snapshot's step)
    [[maybe_unused]] u32x4 in_tags = {0, 0, 0, 0};
    [[maybe_unused]] u32x2 in_nbuf = {0, 0};
    if (DO_STEP) {
        if ((AR || GEN) && !ROLL) in_ep = __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(a.episode + e0, Gc * 4), lane * 4, 0, 0);
        in_scnt = __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(a.step_count + e0, Gc * 4), lane * 4, 0,kInAux);
        if (!PERSIST) in_act = __builtin_amdgcn_raw_buffer_load_b8(make_rsrc(a.actions + v0, NVc), lane, 0,kInAux);   // (PERSIST: granules)
        // (the hooks' visiting order = the caller's dict order, include/mgx.h; one-step kernels: under the load wait too)
        if (HOOKS && !ROLL && a.hook_order) in_hord = __builtin_amdgcn_raw_buffer_load_b8(make_rsrc(a.hook_order + v0, NVc), lane, 0, 0);
        if (cv.has_aux) in_aux = __builtin_amdgcn_raw_buffer_load_b128(make_rsrc(a.aux + e0 * MGX_AUX_BYTES, Gc * MGX_AUX_BYTES), lane16, 0, 0);
    }
    // (2) the tile
    [[maybe_unused]] u32x4 tv[U], tv2[U];
    const bool big_tile = len > 1024 * U;                                   // e.g. one 64x64 env per wavefront
    // Cache policy of the tile loads (template flag STREAM, chosen at launch): a grid tensor that fits the 256 MiB Infinity
    // Cache is re-read from there by the next step and is best left to the default policy; one that does not is a pure
    // stream and is loaded non-temporal (measured: 1 M envs -3.5 % step / -6.5 % gen_obs and C5 -4 % with nt, C4 +3 %).
    // (A launch-time branch around the two forms cost 3-4 % everywhere: the loads must stay in the straight-line burst.)
    constexpr int kTileAux = STREAM ? 2 : 0;
    // DMA instantiations: the tile goes HBM -> LDS directly (buffer_load_dwordx4 ... lds: wave-uniform LDS base in M0 + 16
    // bytes per lane, which is exactly the tile's layout): no staging VGPRs (78 instead of 95: the register peak of the
    // step kernel was this burst), no ds_write pass.  Lanes past the wave's bytes are masked off -- an out-of-range lane
    // would still write its zeros into LDS.  Shorter for a lone wave (-3..5 % up to 2048 wavefronts), but the LDS-DMA path
    // has less throughput than loads + ds_write_b128 (+4 % at 65536 envs): chosen at launch by the number of wavefronts.
    typedef __attribute__((address_space(3))) void *lds_void_ptr;
#define MGX_TILE_BURST(dst, base)                                                                                     \
    if constexpr (DMA) {                                                                                              \
        _Pragma("unroll") for (int u = 0; u < U; ++u)                                                                 \
            if (lane16 + (base) + 1024 * u < len)                                                                     \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(grsrc, (lds_void_ptr)(tile_raw + (base) + 1024 * u), 16, lane16, \
                                                         (base) + 1024 * u, 0, kTileAux);                            \
    } else {                                                                                                          \
        _Pragma("unroll") for (int u = 0; u < U; ++u)                                                                 \
            dst[u] = __builtin_amdgcn_raw_buffer_load_b128(grsrc, lane16 + 1024 * (u & 3), (base) + 4096 * (u >> 2), kTileAux); \
    }
    // MARK_RD: a wavefront whose envs ALL sit on the same pool layout k (their grids in device memory equal pool_grid[k] bit for
    // bit: the marker's promise) takes the layout instead of its envs' grids -- the host asks for the marker only where an env's
    // grid is a power of two of at most 1 KiB (plan_marker_read), so every 16-byte vector of the wavefront's tile is the layout's
    // vector at (16 lane) mod HWB, whichever round of the burst it belongs to: ONE load from a cache-resident line fills them all.
    // The burst itself stays the straight line it is, on both paths (a branch around two forms of it made the wait-count pass
    // drain half the tile in front of the draws below: vmcnt(4) where the straight line has vmcnt(12)): its first load goes
    // through `rs0` -- the grid or the layout --, the other seven through `rs1` -- the grid or a descriptor of NO bytes, whose
    // loads return zeros without touching memory.
    [[maybe_unused]] bool pristine = false;                                  // wave-uniform
    [[maybe_unused]] __amdgpu_buffer_rsrc_t rs0 = grsrc, rs1 = grsrc;
    [[maybe_unused]] int lane16_0 = lane16;
    if constexpr (MARK_RD) {
        // (everything that depends on the marker stays INSIDE this branch: a launch that does not read it must not wait for
        // anything in front of its burst)
        if (read_marker) {
            const int32_t k0 = __builtin_amdgcn_readfirstlane(in_lay);
            pristine = k0 >= 0 && __builtin_amdgcn_ballot_w64(lane < Gc && in_lay != k0) == 0;
            if (pristine) {
                rs0 = make_rsrc(a.pool_grid + (int64_t)k0 * HWB, HWB);
                rs1 = make_rsrc(gsrc, 0);
                lane16_0 = lane16 & (HWB - 1);
            }
        }
    }
    if constexpr (!B3 && PITCH == 0) {                              // (PITCH: the tile is laid out cell by cell, below)
        if constexpr (MARK_RD) {
            tv[0] = __builtin_amdgcn_raw_buffer_load_b128(rs0, lane16_0, 0, kTileAux);
            _Pragma("unroll") for (int u = 1; u < U; ++u)
                tv[u] = __builtin_amdgcn_raw_buffer_load_b128(rs1, lane16 + 1024 * (u & 3), 4096 * (u >> 2), kTileAux);
        } else {
            MGX_TILE_BURST(tv, 0)
        }
    }
    // B3 (byte grids): the first 16 rows of 256 cells -- a C4 wavefront's whole tile -- are requested HERE, with the other formats'
    // tile burst, and converted below once the small inputs are in LDS (round 5's first form issued them after that wait: two
    // memory round trips in a row).  One 12-byte load per lane = 4 cells: a load instruction covers 768 contiguous bytes.
    typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
    constexpr int NR3 = 16;
    [[maybe_unused]] u32x3 w3[B3 ? NR3 : 1];
    // (the buffer's range check is per DWORD: a wavefront's bytes are rounded up to whole dwords -- the bytes behind them are the
    // next wavefront's envs -- except at the very end of the tensor, whose last partial dword is fetched byte by byte below)
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t brs3 =
        make_rsrc(a.grid + e0 * (int64_t)HWG, !B3 ? 0 : (e0 + Gc == a.batch) ? Gc * HWG : ((Gc * HWG + 3) & ~3));
    if constexpr (B3) {
#pragma unroll
        for (int k = 0; k < NR3; ++k) w3[k] = __builtin_amdgcn_raw_buffer_load_b96(brs3, 3 * (4 * lane + 256 * k), 0, kTileAux);
    }
    // (3) P1a of the one-step kernels, while the tile is still on its way: one lane per (env, agent), that agent's draw
    // by jump-ahead (base.py:399); the env's stream after A draws goes straight back to HBM
    uint64_t my_rng[4];
    my_rng[0] = ((uint64_t)in_rngA.y << 32) | in_rngA.x; my_rng[1] = ((uint64_t)in_rngA.w << 32) | in_rngA.z;
    my_rng[2] = ((uint64_t)in_rngB.y << 32) | in_rngB.x; my_rng[3] = ((uint64_t)in_rngB.w << 32) | in_rngB.z;
    uint64_t my_draw = 0;
    [[maybe_unused]] uint64_t post_lo = 0, post_hi = 0;     // GEN: the env's PCG64 state after this step's draws (lane of agent A-1)
    if (DO_STEP && !ROLL && A > 1 && !MGX_DBG((2 | 128)) && lane < NVc) {
        uint64_t jk[4];
        jk[0] = ((uint64_t)in_jmpA.y << 32) | in_jmpA.x; jk[1] = ((uint64_t)in_jmpA.w << 32) | in_jmpA.z;
        jk[2] = ((uint64_t)in_jmpB.y << 32) | in_jmpB.x; jk[3] = ((uint64_t)in_jmpB.w << 32) | in_jmpB.z;
        uint64_t s_lo, s_hi;
        my_draw = pcg64_draw_at(my_rng, jk, s_lo, s_hi);
        if (GEN) { post_lo = s_lo; post_hi = s_hi; }
        if (agent_of_lane == A - 1) { uint64_t *dst = a.rng + (e0 + env_of_lane) * 4; dst[0] = s_lo; dst[1] = s_hi; }
    }
    // (3b) big tiles: a second burst under the same wait (requested here, once the draws' inputs are dead, so that the
    // register peak of P0 stays below that of the gather)
    if (big_tile && !B3) {
        MGX_TILE_BURST(tv2, 1024 * U)
    }
#undef MGX_TILE_BURST
    // (3c) GEN with staging: which episode's successor env `lane`'s slot(s) hold, and env.np_random's 32-bit buffer (gen_state[5]:
    // the draw that picks a candidate may consume it).  STRAIGHT-LINE code, the loads switched off through their buffer's size: with
    // a branch around them the compiler's wait-count pass drained every outstanding load -- the tile -- at the merge, after three
    // dependent kernel-argument fetches: 0.45 us of C3's 8.5 us step (profiles/r5_candidates.txt)
    if constexpr (GEN && MODE == 1) {
        const bool on = DO_STEP && stage_tag != nullptr;
        // (these two loads must STAY the wavefront's newest vector-memory operations: the wait at the end of P0 lets exactly two
        // be outstanding, and the LDS-DMA tile loads -- whose completion only that wait guarantees -- must not be among them)
        asm volatile("" ::: "memory");
        const u32x4 tg = __builtin_amdgcn_raw_buffer_load_b128(make_rsrc(stage_tag + e0 * 4, on ? Gc * 16 : 0), lane * 16, 0, 0);
        in_nbuf = __builtin_amdgcn_raw_buffer_load_b64(make_rsrc(gen_state_p + e0 * 6, (on && cand_K > 1) ? Gc * 48 : 0), lane * 48 + 40, 0, 0);
        asm volatile("" ::: "memory");
        in_tag = on ? (int32_t)tg.x : -1; in_tag_sc = on ? (int32_t)tg.z : -1;
        in_tags = tg;                                   // (candidates: tag[k] = the episode whose successor candidate k is)
    }
    // (4) auto-reset test of the one-step kernels, also under the wait (build-defined, include/mgx.h): one lane per env
    // tests base.py:534-539 on the state the previous step left
    uint64_t reset_mask0 = 0;
    if (AR && DO_STEP && !ROLL) {
        const uint64_t row0 = ((uint64_t)in_row.y << 32) | in_row.x;
        const uint64_t alive = __builtin_amdgcn_ballot_w64(lane < NVc && !row_term(row0));     // bit = (env, agent) slot
        bool done = false;
        if (lane < Gc) {
            const uint64_t amask = (A >= 64) ? ~0ull : ((1ull << A) - 1ull);
            done = (((alive >> mad24(lane, A, 0)) & amask) == 0) | ((int32_t)in_scnt >= a.sp.max_steps);
            if (a.was_reset) a.was_reset[e0 + lane] = (uint8_t)done;
        }
        reset_mask0 = __builtin_amdgcn_ballot_w64(done);
    }
    // (5) the small inputs are here long before the tile: their LDS stores go first
    const uint32_t wall_addr = (uint32_t)(wave * wave_lds_ + cv.wall());
    if (lane == 0) *reinterpret_cast<uint32_t *>(L + cv.wall()) = C8 ? CELL8_WALL : CELL16_WALL;
    if constexpr (C8) {
        // the decode table (mgx_fused.h: LdsCarve::lut): entry (int8)b = cell8_unpack(b); lane l makes the bytes 4l .. 4l+3, which
        // lie side by side in the table: bytes 0..127 in its upper half, 128..255 (= -128..-1) in its lower half
        u32x4 e;
        e.x = cell8_unpack(4u * lane); e.y = cell8_unpack(4u * lane + 1u); e.z = cell8_unpack(4u * lane + 2u); e.w = cell8_unpack(4u * lane + 3u);
        if constexpr (OH) {          // one-hot output: the entry IS the cell's 21-bit one-hot mask (wrappers.py:158-190)
            e.x = one_hot_mask21(e.x); e.y = one_hot_mask21(e.y); e.z = one_hot_mask21(e.z); e.w = one_hot_mask21(e.w);
        }
        *reinterpret_cast<u32x4 *>(L + cv.lut() + ((16 * lane + 512) & 1023)) = e;
    }
    if (lane < NVc) {
        if (DO_STEP && !ROLL && A > 1) rnd[lane] = my_draw;                      // (only the sequential fallback reads the draws)
        reinterpret_cast<u32x2 *>(rows)[lane] = in_row;
        rew[lane] = 0.0;                                                         // base.py:393
        if (DO_STEP) acts[lane] = (int8_t)in_act;
    }
    if (DO_STEP) {
        if (A > 1 && ROLL && lane < Gc * 2) reinterpret_cast<u32x4 *>(rngs)[lane] = in_rngA;
        if (lane < Gc) { scnt[lane] = (int32_t)in_scnt; if (cv.has_aux) reinterpret_cast<u32x4 *>(auxl)[lane] = in_aux; }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                                     // vmcnt(0), for every lane
    if constexpr (B3) {
        // ---- byte grid -> the 16-bit tile.  One 12-byte load per lane = 4 cells, so that a load instruction of the wavefront covers
        // 768 CONTIGUOUS bytes (256 cells; a lane taking 16 cells = 48 bytes per load had every instruction touch 48 cache lines for a
        // third of their bytes each: +11 us at C4 instead of +3); the lane packs its 4 cells (fields, the opaque bit, a box's content)
        // and writes 8 bytes of tile, again contiguous across the wavefront.  Counted on the way, as the pack kernel of the two-launch
        // form does (mgx_pack_grid_env): values the packed format cannot hold; the ring below.
        const int ncell = Gc * H * W;
        const bool tensor_end = e0 + Gc == a.batch;
        int nbad = 0;
        constexpr int NR = NR3;                                      // rows of 256 cells in flight: 4096 cells = a C4 wavefront's 16 envs
        for (int c0 = 4 * lane; c0 < ncell; c0 += 256 * NR) {
            if (c0 != 4 * lane) {                                    // (the first rows were requested before the small inputs' wait)
#pragma unroll
                for (int k = 0; k < NR; ++k) w3[k] = __builtin_amdgcn_raw_buffer_load_b96(brs3, 3 * (c0 + 256 * k), 0, kTileAux);
            }
            // Four cells at a time on byte PLANES (v_perm_b32 de-interleaves the 12 bytes into their four types, colours and states);
            // "this byte == K" / "!= 0" are exact per-byte tests without carries between the bytes:
            //   zero(x) = ~(((x & 0x7f..) + 0x7f..) | x | 0x7f..)  ->  0x80 in every byte of x that is 0
            // 32 instructions per 4 cells, no branch (cell by cell: 59 and a ballot per row; a C4 wavefront converts 16 rows per lane).
            uint32_t cont = 0;                                       // state bytes with bits above the state: boxes that hold something
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                if (c0 + 256 * k - 4 * lane >= ncell) break;                     // (wave-uniform: no lane has cells in this row)
                const uint32_t w0 = w3[k].x, w1 = w3[k].y, w2 = w3[k].z;      // [t0 c0 s0 t1] [c1 s1 t2 c2] [s2 t3 c3 s3]
                const uint32_t T4 = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, 0x00060300u), 0x05020100u);
                const uint32_t C4 = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, 0x00070401u), 0x06020100u);
                const uint32_t S4 = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, 0x00000502u), 0x07040100u);
                auto zero80 = [](const uint32_t x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); };
                const uint32_t S3 = S4 & 0x03030303u;
                const uint32_t shut = (S3 + 0x7f7f7f7fu) & 0x80808080u;                         // state != open
                const uint32_t opq = zero80(T4 ^ (0x01010101u * (uint32_t)T_WALL))
                                   | (zero80(T4 ^ (0x01010101u * (uint32_t)T_DOOR)) & shut);      // obs.py:46-63, in bit 7 of each byte
                const uint32_t L4 = T4 & 0x0f0f0f0fu;                                           // cell bits 7..0: the type
                const uint32_t H4 = (C4 & 0x07070707u) | (S3 << 4) | opq;                       // bits 15..8: colour, state, opaque
                nbad += ((T4 & 0xf0f0f0f0u) | (C4 & 0xf8f8f8f8u)) != 0;     // a type > 15 or a colour > 7 among these 4 cells
                cont |= S4 & 0xfcfcfcfcu;
                const int cc = c0 + 256 * k;
                if (2 * cc < Gc * HWB) {
                    MGX_CHECK_LDS_PTR(1, tile_raw + 2 * cc, 8);
                    *reinterpret_cast<u32x2 *>(tile_raw + 2 * cc) =
                        u32x2{__builtin_amdgcn_perm(H4, L4, 0x05010400u), __builtin_amdgcn_perm(H4, L4, 0x07030602u)};
                }
            }
            if (MGX_ANY_LANE(cont != 0)) {                                   // rare: the rows again, cell by cell, with their contents
#pragma unroll
                for (int k = 0; k < NR; ++k) {
                    if (c0 + 256 * k - 4 * lane >= ncell) break;
                    const uint32_t w0 = w3[k].x, w1 = w3[k].y, w2 = w3[k].z;
                    const uint32_t c[4] = {w0 & 0xffffffu, __builtin_amdgcn_alignbyte(w1, w0, 3) & 0xffffffu,
                                           __builtin_amdgcn_alignbyte(w2, w1, 2) & 0xffffffu, w2 >> 8};
                    if (!MGX_ANY_LANE(((c[0] | c[1] | c[2] | c[3]) >> 18) != 0)) continue;
                    uint32_t p[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        p[j] = cell_pack(c[j]);
                        nbad += ((c[j] >> 18) != 0) & (((c[j] & 0xffu) != (uint32_t)T_BOX) | (((c[j] >> 18) & 7u) == 0) | ((c[j] >> 21) > 5u));
                    }
                    const int cc = c0 + 256 * k;
                    if (2 * cc < Gc * HWB) *reinterpret_cast<u32x2 *>(tile_raw + 2 * cc) = u32x2{p[0] | (p[1] << 16), p[2] | (p[3] << 16)};
                }
            }
        }
        if (tensor_end && ((Gc * HWG) & 3) != 0 && lane < 2) {           // the cells that reach into the tensor's last, partial dword
            const int cell = ncell - 1 - lane;
            if (cell >= 0) store_cell16(tile_raw + 2 * cell, cell_pack(load_obs_cell(a.grid + e0 * (int64_t)HWG + 3 * cell)));
        }
        int32_t *const gbad = MGX_LATE(grid_bad);
        if (gbad) {
            wave_sync();
            // the outer ring of every env must be WALL (include/mgx.h PRECONDITION).  A lane owns ring POSITION p (the top row, the
            // bottom row, then the left / right cells of the rows between), decoded once; it then looks at that cell of every env of
            // the wavefront -- four independent LDS reads in flight.  (First form: lanes = 4 envs x 16 edge positions, four dependent
            // reads per env group: 1.35 us of C4's 24 us step, profiles/r5_candidates.txt)
            int nring = 0;
            const int ringN = 2 * W + 2 * (H - 2);
            for (int p = lane; p < ringN; p += 64) {
                const int q = p - 2 * W;
                const int y = p < W ? 0 : (q < 0 ? H - 1 : 1 + (q >> 1));
                const int x = p < W ? p : (q < 0 ? p - W : ((q & 1) ? W - 1 : 0));
                const uint8_t *cp = tile_raw + 2 * (y * W + x);
                int e = 0;
                for (; e + 4 <= Gc; e += 4) {
                    const uint32_t r0 = load_cell16(cp + e * HWB), r1 = load_cell16(cp + (e + 1) * HWB),
                                   r2 = load_cell16(cp + (e + 2) * HWB), r3 = load_cell16(cp + (e + 3) * HWB);
                    nring += (r0 != CELL16_WALL) + (r1 != CELL16_WALL) + (r2 != CELL16_WALL) + (r3 != CELL16_WALL);
                }
                for (; e < Gc; ++e) nring += load_cell16(cp + e * HWB) != CELL16_WALL;
            }
            if (nbad) atomicAdd(gbad, nbad);
            if (nring) atomicAdd(gbad + 1, nring);
        }
    } else
    if constexpr (!DMA && PITCH == 0) {
        if (MARK_RD && pristine) {              // the one layout vector, into every env's tile (behind the wait: no wait count differs)
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (lane16 + 1024 * u < len) {
                    MGX_CHECK_LDS_PTR(1, tile_raw + lane16 + 1024 * u, 16);
                    *reinterpret_cast<u32x4 *>(tile_raw + lane16 + 1024 * u) = tv[0];
                }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (lane16 + 1024 * u < len) {
                    MGX_CHECK_LDS_PTR(1, tile_raw + lane16 + 1024 * u, 16);
                    *reinterpret_cast<u32x4 *>(tile_raw + lane16 + 1024 * u) = tv[u];
                }
        }
    }
    if (big_tile && !B3) {
        if constexpr (!DMA) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (lane16 + 1024 * (U + u) < len) *reinterpret_cast<u32x4 *>(tile_raw + lane16 + 1024 * (U + u)) = tv2[u];
        }
        for (int rel = lane16 + 2048 * U; rel < len; rel += 1024)               // tiles larger than two bursts (16 KiB)
            *reinterpret_cast<u32x4 *>(tile_raw + rel) = __builtin_amdgcn_raw_buffer_load_b128(grsrc, rel, 0, kTileAux);
    }
    if (!B3 && g1 == gtotal && (gtotal & 15)) {                   // last, partial 16-byte vector of the tensor
        const int64_t t0 = gtotal & ~(int64_t)15;
        for (int k = lane; k < (int)(gtotal & 15); k += 64) tile_raw[(int)(t0 - ga) + k] = a.grid[t0 + k];
    }
    // (the loops above may have loaded.)  GEN with candidates: the tag / np_random-buffer loads of (3c) -- the wavefront's NEWEST
    // vector-memory operations, read-only data that comes from further away than the tile the previous step wrote -- are only
    // needed once an episode ends: vmcnt counts in order, so "all but the newest two" is everything P1 needs
    if (GEN && MODE == 1 && cand_K > 0) __builtin_amdgcn_s_waitcnt(0x0F72);
    else __builtin_amdgcn_s_waitcnt(0x0F70);
    wave_sync();

    // The names a step uses for "its" envs, re-declared for slice S of the wavefront (NS == 1: the same values again)
#define MGX_SLICE_VARS(S)                                                                                               \
    [[maybe_unused]] const int64_t e0 = e0w + (int64_t)(S) * Gw_;                                                       \
    [[maybe_unused]] const int Gc = (int)min((int64_t)Gw_, a.batch - e0);                                               \
    [[maybe_unused]] const int NVc = Gc * A;                                                                            \
    [[maybe_unused]] const int64_t v0 = e0 * A;                                                                         \
    [[maybe_unused]] uint64_t *const rows = reinterpret_cast<uint64_t *>(L + cv.rows(S));                               \
    [[maybe_unused]] uint64_t *const rngs = reinterpret_cast<uint64_t *>(L + cv.rng(S));                                \
    [[maybe_unused]] int32_t *const scnt = reinterpret_cast<int32_t *>(L + cv.scnt(S));                                 \
    [[maybe_unused]] uint4 *const auxl = reinterpret_cast<uint4 *>(L + cv.aux(S));                                      \
    [[maybe_unused]] const int64_t g0 = e0 * HWB, g1 = g0 + (int64_t)Gc * HWB;                                          \
    [[maybe_unused]] const int64_t ga = B3 ? g0 : (g0 & ~(int64_t)15);                                                  \
    [[maybe_unused]] uint8_t *const tile_raw = L + cv.tile(S);                                                          \
    [[maybe_unused]] const int tile_skew = (int)(g0 - ga);                                                              \
    [[maybe_unused]] uint8_t *const tile = tile_raw + tile_skew;                                                        \
    [[maybe_unused]] const int len = (int)(g1 - ga);
    // the tile in the ring-sharing layout (PITCH): cell (x, y) of env e at (e * PITCH * (H - 1) + y * PITCH + x) * CB -- column W - 1 of a
    // row IS column 0 of the next, the last row of an env IS the first of the next: all WALL (include/mgx.h PRECONDITION; the host
    // checks it where grids enter), so lanes that store to a shared cell store the same value.  Once per launch: plain loops.
    [[maybe_unused]] auto load_pitch_tile = [&](uint8_t *const t_raw, const int64_t env0, const int nenv) {
        const uint16_t *src = reinterpret_cast<const uint16_t *>(a.grid + env0 * HWB);
        const int HW = H * W;
        for (int c = lane; c < nenv * HW; c += 64) {
            const int e = c / HW, r = c - e * HW, y = r / W, x = r - y * W;
            reinterpret_cast<uint16_t *>(t_raw)[e * PITCH * (H - 1) + y * PITCH + x] = src[c];
        }
    };
    if constexpr (PITCH != 0) {
        static_assert(PITCH == 0 || (CB == 2 && ROLL), "ring-sharing tiles: 16-bit cells, rollout / persistent kernels");
        load_pitch_tile(tile_raw, e0, Gc);
        wave_sync();
    }
    if constexpr (NS > 1) {
        // ---- the other slices' state: HBM -> LDS, once per launch (plain loops: this is not the step)
        static_assert(NS == 1 || (kShapes[SHAPE].W * kShapes[SHAPE].H * CB * kShapes[SHAPE].Gw) % 16 == 0, "slices: whole 16-byte vectors per slice");
        for (int s1 = 1; s1 < ns_act; ++s1) {
            MGX_SLICE_VARS(s1)
            if constexpr (PITCH != 0) {
                load_pitch_tile(tile_raw, e0, Gc);
            } else {
                const __amdgpu_buffer_rsrc_t gr1 = make_rsrc(a.grid + g0, Gc * HWB);
                for (int rel = lane16; rel < len; rel += 1024)
                    *reinterpret_cast<u32x4 *>(tile_raw + rel) = __builtin_amdgcn_raw_buffer_load_b128(gr1, rel, 0, 0);
            }
            if (lane < NVc) rows[lane] = reinterpret_cast<const uint64_t *>(a.agents)[v0 + lane];
            if (DO_STEP) {
                if (A > 1 && lane < Gc * 2)
                    reinterpret_cast<u32x4 *>(rngs)[lane] = __builtin_amdgcn_raw_buffer_load_b128(make_rsrc(a.rng + e0 * 4, Gc * 32), lane16, 0, 0);
                if (lane < Gc) {
                    scnt[lane] = a.step_count[e0 + lane];
                    if (cv.has_aux) auxl[lane] = reinterpret_cast<const uint4 *>(a.aux)[e0 + lane];
                }
            }
        }
        wave_sync();
    }

    // GEN with staging: an env that TRUNCATES with this step and whose slot holds its episode's successor will adopt it in the tail
    // (include/mgx.h: MgxGenStage) -- all of that is known here, so the slot's content is requested NOW and arrives under the step
    // (the first such env of the wavefront; a second one -- rare -- loads in the tail).  Nothing writes a slot while its tag names
    // the env's current episode.
    [[maybe_unused]] int pre_e = -1;
    [[maybe_unused]] uint32_t pre_grid[4] = {0, 0, 0, 0};
    [[maybe_unused]] uint64_t pre_row = 0, pre_word = 0;
    [[maybe_unused]] uint4 pre_aux = {0, 0, 0, 0};
    if constexpr (GEN && MODE == 1) {
        if (stage_tag && cand_K == 0) {
            const int32_t lead0 = MGX_LATE_STAGE(lead);
            const bool will = lane < Gc && in_tag == (int32_t)in_ep && (int32_t)in_scnt + 1 == a.sp.max_steps
                              && in_tag_sc == a.sp.max_steps - lead0;
            const uint64_t pm = __builtin_amdgcn_ballot_w64(will);
            if (pm != 0 && (HWB & 3) == 0 && HWB <= 1024) {
                pre_e = __builtin_ctzll(pm);
                const int64_t b = e0 + pre_e;
                const uint32_t *sg = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(MGX_LATE_STAGE(grid)) + b * HWB);
                const int nd = HWB / 4;
#pragma unroll
                for (int k = 0; k < 4; ++k) pre_grid[k] = (lane + 64 * k < nd) ? sg[lane + 64 * k] : 0u;
                pre_row = lane < A ? (reinterpret_cast<const uint64_t *>(MGX_LATE_STAGE(agents)) + b * A)[lane] : 0ull;
                pre_word = lane < 10 ? (MGX_LATE_STAGE(words) + b * 12)[lane] : 0ull;
                if (HOOKS) pre_aux = reinterpret_cast<const uint4 *>(MGX_LATE_STAGE(aux))[b];
            }
        }
    }
    [[maybe_unused]] uint64_t cand_mask = 0;
    [[maybe_unused]] int cand_r = 0;                                        // env `lane`'s draw and np_random after it: made once,
    [[maybe_unused]] mgx_gen::NpGen cand_npr = {};                          // after the rules phase; the tail stores them
    [[maybe_unused]] bool done_now = false;                                 // GEN: env `lane`'s episode ends with this step
    [[maybe_unused]] uint64_t done_mask = 0;
    [[maybe_unused]] auto cand_draw = [&](mgx_gen::NpGen &npr) -> int {     // all lanes; lane e < Gc: env e's draw (0-based)
        if (cand_K <= 1) return 0;
        const int el = lane < Gc ? lane : 0, src_last = (el * A + (A - 1)) * 4, src_first = el * A * 4;
        auto take64 = [&](const uint64_t v, const int src) -> uint64_t {
            return ((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(v >> 32)) << 32)
                 | (uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)v);
        };
        npr.s[0] = take64(post_lo, src_last); npr.s[1] = take64(post_hi, src_last);
        npr.s[2] = take64(my_rng[2], src_first); npr.s[3] = take64(my_rng[3], src_first);
        npr.buf = ((uint64_t)in_nbuf.y << 32) | in_nbuf.x;
        return mgx_gen::np_integers(npr, 1, MGX_LATE_GEN(room_size) - 1) - 1;       // roomgrid.py:104-106
    };
    MGX_MARK("P0end");
    // lane constants: cell k = lane + 64*it  <->  image[i][j], k = j*V + i (depth-row major, so each ballot
    // word holds whole visibility rows); lateral offset la = i - V/2, forward distance fw = V-1-j.
    auto lane_consts = [&]() {
        LaneConst<V, NW> c;
#pragma unroll
        for (int it = 0; it < NW; ++it) {
            const int k = lane + 64 * it;
            const int j = k / V, i = k - j * V;
            c.act[it] = k < V2;
            c.pk[it] = ((uint32_t)(V - 1 - j) & 0xffffu) | ((uint32_t)(i - V / 2) << 16);   // (fw, la)
            c.q3[it] = (i * V + j) * 3;
            c.own[it] = (i == V / 2) && (j == V - 1);
        }
        c.sub16 = 0;
        if constexpr (PK3) {
            // the shared remainder passes (mgx_fused.h: kPack3): lane = (view `sub` of the pass, cell 64 + lane % R of that view)
            constexpr int R = V2 - 64;
            const int sub = min((lane * ((65536 + R - 1) / R)) >> 16, 2), k = 64 + lane - sub * R;   // (lanes >= 3 R: inactive)
            const int j = k / V, i = k - j * V;
            c.act[1] = lane < 3 * R;
            c.pk[1] = ((uint32_t)(V - 1 - j) & 0xffffu) | ((uint32_t)(i - V / 2) << 16);
            c.q3[1] = (i * V + j) * 3 + sub * (V2 * 3);
            c.own[1] = false;
            c.sub16 = sub * (int)sizeof(ViewRec);
        }
        return c;
    };
    LaneConst<V, NW> lc_roll;
    if (ROLL) lc_roll = lane_consts();            // hoisted out of the step loop; the one-step kernels make them late

    StepCfg cf = make_cfg(a.sp);
    cf.cb = CB;
    if (FIXED) { cf.W = W; cf.H = H; cf.A = A; cf.P = PITCH ? PITCH : W; }
    const int T = ROLL ? a.T : 1;
    const int64_t BA = a.batch * A;
    int8_t next_act = 0;                                                     // ROLL: next step's action, in flight
    if (ROLL && !PERSIST && lane < NVc) next_act = a.actions[v0 + lane];
    [[maybe_unused]] int steps_done = 0;                                     // PERSIST: steps this wavefront completed
    // (NS > 1: the loop runs over (step, slice) pairs -- step t of slice 0, step t of slice 1, step t + 1 of slice 0, ...)
    const int n_ts = NS > 1 ? T * ns_act : T;
    for (int ts = 0; ts < n_ts; ++ts) {
    const int t = NS > 1 ? (ns_act > 1 ? ts >> 1 : ts) : ts;
    [[maybe_unused]] const int sl_s = NS > 1 ? (ns_act > 1 ? (ts & 1) : 0) : 0;
    // (the ring-sharing resident shape only: the lane index is made opaque once per step, so that what is derived from it is
    // recomputed per step instead of being hoisted out of the loop and held in registers across it.  On the other resident shapes it
    // measured 153 -> 143 VGPRs on the one-slice kernel -- and 2-3 % SLOWER, same box (profiles/r6_resident.txt): at 12 wavefronts per
    // CU the LDS, not the registers, bounds the occupancy, so the recomputation buys nothing.)
    if constexpr (RSHAPE && PITCH != 0) asm volatile("" : "+v"(lane_));   // (kShapes 9: what makes 127 VGPRs spill-free)
    MGX_SLICE_VARS(sl_s)
    // (PERSIST writes every step's outputs to the same rows.  On the ring-sharing resident shape the offset is made opaque per step:
    // loop-invariant, the ten output descriptors are hoisted out of the step loop and HELD -- 190 spilled SGPRs, which take four
    // VGPRs' lanes and push two real VGPRs of the 128 into scratch)
    [[maybe_unused]] int t_out = 0;
#if !MGX_TIMESTAMPS          // (the stamps build: hipcc 7.2's register allocator crashes on one of its persistent kernels with this in place)
    if constexpr (PERSIST) asm volatile("" : "+s"(t_out));
#endif
    const int64_t tv0 = (PERSIST ? (int64_t)t_out : (int64_t)t * BA) + v0;   // this step's (env, agent) output rows
    const int64_t tb0 = PERSIST ? (int64_t)t_out : (int64_t)t * a.batch;     // ... and its per-env output rows
    if constexpr (PERSIST) {
        // ------------------------------------------------------------ the step's actions: one 8-byte granule per 4 agents of an
        // env, {tag = t + 1, 4 action bytes}, each written by ONE agent-scope store of the producer -- the data is the flag.  The
        // wavefront re-reads ITS granules (relaxed agent loads: no fence, no other wavefront's traffic) until every tag matches;
        // every 16th pass it also looks at the stop word and at the clock (bounded spin: a producer that went away must not hang
        // the device).
        const int gpe = (A + 3) >> 2, ng = Gc * gpe;                          // granules per env / of this wavefront (<= 32)
        const uint64_t *gr = a.granules + e0 * gpe;
        const uint32_t want = (uint32_t)t + 1u;
        uint64_t g = 0;
        bool leave = false;
        const uint64_t t_wait0 = __builtin_amdgcn_s_memrealtime();
        for (uint32_t spin = 1;; ++spin) {
            if (lane < ng) g = __hip_atomic_load(gr + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__builtin_amdgcn_ballot_w64(lane < ng && (uint32_t)(g >> 32) != want) == 0) break;
            if ((spin & 15u) == 0) {
                const uint32_t stop = __hip_atomic_load(a.pctrl + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool late = __builtin_amdgcn_s_memrealtime() - t_wait0 > (uint64_t)a.timeout_ticks;
                if (__builtin_amdgcn_readfirstlane(stop) != 0 || late) {
                    if (late && lane == 0) atomicAdd(a.pctrl + 1, 1u);           // (timeouts: the caller reads it after the launch)
                    leave = true;
                    break;
                }
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (leave) break;
#if MGX_SPANS
        // (spans build: record span_base + t * wavefronts + wid = [actions seen, flag published] of this wavefront's step t)
        const int64_t span_rec = a.span_base + (int64_t)t * gridDim.x * (blockDim.x >> 6) + wid;
        if (lane == 0 && span_rec < kSpanCap) g_span[2 * span_rec] = __builtin_amdgcn_s_memrealtime();
#endif
        if (lane < ng) {
            const int e = lane / gpe, q = lane - e * gpe;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < A) acts[e * A + 4 * q + j] = (int8_t)(g >> (8 * j));
        }
        if (lane < NVc) rew[lane] = 0.0;
        wave_sync();
    } else if (ROLL) {
        if (lane < NVc) { acts[lane] = next_act; rew[lane] = 0.0; }
        if constexpr (NS > 1) {                                                  // the next (step, slice) of the sequence
            const bool wrap = sl_s + 1 >= ns_act;
            const int t_n = wrap ? t + 1 : t;
            const int64_t e0_n = e0w + (wrap ? 0 : (int64_t)(sl_s + 1) * Gw_);
            const int NVc_n = (int)min((int64_t)Gw_, a.batch - e0_n) * A;
            if (t_n < T && lane < NVc_n) next_act = a.actions[(int64_t)t_n * BA + e0_n * A + lane];
        } else {
            if (t + 1 < T && lane < NVc) next_act = a.actions[(int64_t)(t + 1) * BA + v0 + lane];
        }
        wave_sync();
    }
    uint32_t ovl_saved = 0;                                                  // ROLL: clean cell under this agent's overlay
    int ovl_off = -1;
    // this lane's agent row, carried in registers through the step (one-step kernels have it from P0); re-read from LDS
    // only after something else may have changed it (a reset, the sequential fallback, an env hook)
    uint64_t cur_row = ROLL ? (lane < NVc ? rows[lane] : 0ull) : (((uint64_t)in_row.y << 32) | in_row.x);
    MGX_MARK("AR");
    uint64_t reset_mask = 0;                                                 // AR: envs (bit = env of the wave) restarted now
    if (AR && DO_STEP) {
        // -------------------------------------------------------------- auto-reset: a finished env takes the pool layout
        // (first_env + b + episode * 7919) mod K, step_count 0, episode + 1 -- the definition mgx_reset_done implements
        if (ROLL) {
            const uint64_t alive = __builtin_amdgcn_ballot_w64(lane < NVc && !row_term(cur_row));   // bit = (env, agent) slot
            bool done = false;
            if (lane < Gc) {
                const uint64_t amask = (A >= 64) ? ~0ull : ((1ull << A) - 1ull);
                done = (((alive >> mad24(lane, A, 0)) & amask) == 0) | (scnt[lane] >= cf.max_steps);
                if (a.was_reset) MGX_PUB_STORE_U8(a.was_reset + tb0 + e0, lane, Gc, done);
            }
            reset_mask = __builtin_amdgcn_ballot_w64(done);
        } else {
            reset_mask = reset_mask0;                                            // (tested in P0, under the load wait)
        }
        MGX_SPAN_FLAG(1, reset_mask != 0);
        if (reset_mask != 0) {                                                   // rare: a few envs per thousand steps
            MGX_RARE_PATH_PRIO();
            // every restarting env's episode count and layout index, one lane per env: on the vector unit (the scalar form of
            // the 64-bit arithmetic cost the whole kernel six more spilled SGPRs)
            int32_t *p_ep = MGX_LATE(episode);
            int32_t my_ep = 0, my_lay = 0;
            if (lane < Gc && ((reset_mask >> lane) & 1ull)) {
                // (one-step kernels fetched the episode counts in P0: no dependent load in front of the copy)
                my_ep = ROLL ? p_ep[e0 + lane] : (int32_t)in_ep;
                my_lay = pool_index(MGX_LATE(first_env), e0 + lane, my_ep, MGX_LATE(pool_size), MGX_LATE(pool_magic));
            }
            for (uint64_t m = reset_mask; m != 0; m &= m - 1) {
                const int e = __builtin_ctzll(m);                                // wave-uniform
                const int64_t b = e0 + e;
                const int32_t ep = (int32_t)__builtin_amdgcn_readlane(my_ep, e);
                const int lay = (int)__builtin_amdgcn_readlane(my_lay, e);
                wave_sync();
                if (lane == 0) p_ep[b] = ep + 1;
                if constexpr (MARK) {                                            // the env's grid IS layout `lay` from here on (the copy
                    int32_t *const p_lay = MGX_LATE(grid_layout);                // below); a cell written later in this step stores -1
                    if (p_lay && lane == 0) p_lay[b] = lay;                      // behind it, in program order
                }
                const uint8_t *sg = MGX_LATE(pool_grid) + (int64_t)lay * HWG;
                uint8_t *etile = tile + e * TSB;
                uint8_t *gg = MGX_LATE(grid) + b * HWG;
                const uint32_t etile_addr = (uint32_t)(uintptr_t)(lds_u32_ptr)etile;
                // Everything the restart reads is requested before anything is stored: the layout's agent rows, its hook state
                // and the first KiB of its grid come back in ONE round trip (a load issued behind the stores of a previous
                // chunk also waits for those stores: vmcnt counts them).  This wavefront is the launch's slowest.
                const uint64_t *sa = reinterpret_cast<const uint64_t *>(MGX_LATE(pool_agents)) + (int64_t)lay * A;
                const uint64_t nrow = lane < A ? sa[lane] : 0ull;                // (A <= 32: one pass)
                uint4 naux = {0, 0, 0, 0};
                if (HOOKS) naux = reinterpret_cast<const uint4 *>(MGX_LATE(pool_aux))[lay];
                if constexpr (PITCH != 0) {
                    // ring-sharing tile: the layout's cells one by one (the rollout / persistent kernels write the grid back at the end)
                    for (int i = lane; i < H * W; i += 64) {
                        const int y = i / W, x = i - y * W;
                        reinterpret_cast<uint16_t *>(etile)[y * PITCH + x] = reinterpret_cast<const uint16_t *>(sg)[i];
                    }
                } else
                if constexpr (B3) {
                    // byte grids: the layout's triples go to the env's grid as they are (dwords when everything is aligned) and,
                    // packed, into the tile
                    if (((HWG | (uint32_t)reinterpret_cast<uintptr_t>(sg) | (uint32_t)reinterpret_cast<uintptr_t>(gg)) & 3u) == 0) {
                        const int nd = HWG / 4;
                        for (int i = lane; i < nd; i += 64) reinterpret_cast<uint32_t *>(gg)[i] = reinterpret_cast<const uint32_t *>(sg)[i];
                    } else {
                        for (int i = lane; i < HWG; i += 64) gg[i] = sg[i];
                    }
                    for (int i = lane; i < H * W; i += 64) store_cell16(etile + 2 * i, cell_pack(load_obs_cell(sg + 3 * i)));
                } else
                if (BIGCOPY && HWB >= 4096 && ((HWB | etile_addr | (uint32_t)reinterpret_cast<uintptr_t>(sg) | (uint32_t)reinterpret_cast<uintptr_t>(gg)) & 15u) == 0) {
                    // big layouts (C5: 8 KiB): 16-byte vectors, four per lane in flight -- 4 KiB per round trip instead of 1 KiB
                    // (the dword loop below made this wavefront the launch's slowest by +13 us)
                    const int nv = HWB / 16;
                    for (int base = lane; base < nv; base += 256) {
                        uint4 v4[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            v4[k] = (base + 64 * k < nv) ? reinterpret_cast<const uint4 *>(sg)[base + 64 * k] : uint4{0, 0, 0, 0};
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (base + 64 * k < nv) {
                                reinterpret_cast<uint4 *>(etile)[base + 64 * k] = v4[k];
                                if (!ROLL) reinterpret_cast<uint4 *>(gg)[base + 64 * k] = v4[k];
                            }
                    }
                } else if (((HWB | etile_addr | (uint32_t)reinterpret_cast<uintptr_t>(sg) | (uint32_t)reinterpret_cast<uintptr_t>(gg)) & 3u) == 0) {
                    const int nd = HWB / 4;
                    uint32_t v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = (lane + 64 * k < nd) ? reinterpret_cast<const uint32_t *>(sg)[lane + 64 * k] : 0u;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (lane + 64 * k < nd) {
                            reinterpret_cast<uint32_t *>(etile)[lane + 64 * k] = v[k];
                            if (!ROLL) reinterpret_cast<uint32_t *>(gg)[lane + 64 * k] = v[k];   // (the rollout writes its tile back at the end)
                        }
#pragma unroll 4
                    for (int i = lane + 256; i < nd; i += 64) {                  // grids beyond 1 KiB: several loads in flight per lane
                        const uint32_t w = reinterpret_cast<const uint32_t *>(sg)[i];
                        reinterpret_cast<uint32_t *>(etile)[i] = w;
                        if (!ROLL) reinterpret_cast<uint32_t *>(gg)[i] = w;
                    }
                } else {
                    for (int i = lane; i < HWB; i += 64) {                       // bytes: layouts of any size / alignment
                        const uint8_t w = sg[i];
                        etile[i] = w;
                        if (!ROLL) gg[i] = w;
                    }
                }
                if (lane < A) rows[e * A + lane] = nrow;
                if (lane == 0) {
                    scnt[e] = 0;
                    if (HOOKS) {
                        auxl[e] = naux;
                        if (!ROLL) reinterpret_cast<uint4 *>(MGX_LATE(aux))[b] = naux;
                    }
                }
            }
            wave_sync();
            if (!ROLL && lane < Gc && ((reset_mask >> lane) & 1ull)) in_scnt = 0;
        }
    }
    if (AR && reset_mask != 0 && lane < NVc) cur_row = rows[lane];
    double my_rew = 0.0;                                                     // this agent's reward (base.py:393), in a register
    if (DO_STEP && !MGX_DBG(2)) {
        const bool in = lane < NVc;
        // (fetched now so that the s_load latency hides behind P1a / P1s)
        int32_t *const p_step_count = ROLL ? nullptr : MGX_LATE(step_count);
        uint8_t *const p_truncated = MGX_LATE(truncated);
        MGX_MARK("P1a");
        if (ROLL && A > 1 && !MGX_DBG(128)) {
            // -------------------------------------------------------------- P1a (rollout; the one-step kernels did it in P0):
            // one lane per (env, agent): its draw
            if (in) {
                const int e = env_of_lane, ai = agent_of_lane;
                uint64_t s_lo, s_hi;
                rnd[lane] = pcg64_draw_at(rngs + e * 4, jump + ai * 4, s_lo, s_hi);         // base.py:399
                if (ai == A - 1) { rngs[e * 4 + 0] = s_lo; rngs[e * 4 + 1] = s_hi; }        // (every lane has read it: in-order LDS)
            }
        }
        MGX_MARK("P1s");
        // ------------------------------------------------------------------ P1s: one lane per (env, agent): order-free
        // evaluation of every agent's action against the pre-step state (mgx_rules.h: conditions (1)-(3))
        int32_t *woff = reinterpret_cast<int32_t *>(L + cv.woff());             // [slot]
        AgentEval ev{};
        uint8_t *mytile = tile + env_of_lane * TSB;
        if (in) MGX_CHECK_LDS_PTR(2, mytile, TSB);
        if (in && !MGX_DBG(64)) {
            const int so = (env_kind == MGX_KIND_REDBLUEDOORS)
                               ? stale_offset(cf, reinterpret_cast<const uint8_t *>(auxl + env_of_lane), env_kind) : -1;
            ev = eval_agent(cf, mytile, rows + env_of_lane * A, ROLL ? (int)acts[lane] : (int)(int8_t)in_act, cur_row, true, so);
        }
        // condition (2) needs the cells the other agents write: exchanged through LDS only when somebody writes at all
        bool conf = false;
        MGX_SPAN_FLAG(8, __builtin_amdgcn_ballot_w64(in && ev.writes) != 0);
        const bool any_writes = __builtin_amdgcn_ballot_w64(in && ev.writes) != 0;     // (wave-uniform: `woff` is valid)
        if (any_writes) {
            if (in) woff[lane] = ev.writes ? ev.off : -1;
            wave_sync();
            conf = in && spec_cell_conflict(woff + env_of_lane * A, A, agent_of_lane, ev);
        }
        // the common step has none of this in the whole wavefront: one ballot decides whether the masks are needed at all
        bool fb = false, does_act = in;
        uint64_t m_ends = 0, m_evt = 0, genv = 0;
        if (__builtin_amdgcn_ballot_w64(in && (ev.bad | conf | ev.used_presence | ev.success | ev.failure)) != 0) {
            MGX_RARE_PATH_PRIO();
            const uint64_t m_bad = __builtin_amdgcn_ballot_w64(in && ev.bad);
            const uint64_t m_conf = __builtin_amdgcn_ballot_w64(conf);
            const uint64_t m_pres = __builtin_amdgcn_ballot_w64(in && ev.used_presence);
            const uint64_t m_moved = __builtin_amdgcn_ballot_w64(in && ev.moved);
            m_ends = __builtin_amdgcn_ballot_w64(in && event_ends_all(cf, ev));
            m_evt = __builtin_amdgcn_ballot_w64(in && (ev.success | ev.failure));
            const uint64_t amask = (A >= 64) ? ~0ull : ((1ull << A) - 1ull);
            genv = in ? (amask << (env_of_lane * A)) : 0ull;                     // the lanes of this lane's env
            fb = in && spec_needs_fallback(m_bad & genv, m_conf & genv, m_pres & genv, m_moved & genv);
            // an event that ends the episode for every agent: only the agents visited up to it act (mgx_rules.h)
            does_act = in && !fb;
            const uint64_t m_fb = __builtin_amdgcn_ballot_w64(fb);
            if (A > 1 && (m_ends | m_fb) != 0) {                                 // rare, wave-uniform
                int my_rank = 0;
                if (in) {
                    my_rank = draw_rank(rnd + env_of_lane * A, A, agent_of_lane);
                    ord[env_of_lane * A + my_rank] = (uint8_t)agent_of_lane;
                }
                wave_sync();
                if (in && (m_ends & genv) != 0)
                    does_act = does_act && my_rank <= event_cutoff(ord + env_of_lane * A, (m_ends & genv) >> (env_of_lane * A), A);
                // An env that takes the sequential loop: the agents visited BEFORE the first one whose inputs an earlier agent
                // changes (mgx_rules.h: prefix_blocked) still see the pre-step state they were evaluated against -- they commit
                // here with everybody else, and the loop (P1c: one lane walking through the agents, ~0.85 us each) starts at that
                // cutoff.  A launch lasts as long as its slowest wavefront: at C5 a 16-agent env in the loop was +10 us, at
                // 16384 BlockedUnlockPickup envs 3 % of the wavefronts come through here every step.
                // (PREFIX: compiled into the kernels that serve many-agent envs; the throughput instantiations for small views --
                // the C4 headline -- and the 2-agent shapes keep the first-agent shortcut: measured, the general form costs them
                // +1..2.5 % in registers and rare-path instructions and buys nothing at A <= 4)
                if constexpr (PREFIX) {
                    if (m_fb != 0 && A > 2) {
                        // every agent of a fallback env marks its own entry of the visiting order "blocked" (bit 6); the env's
                        // cutoff = the first marked entry; the entries below it are done (bit 7)
                        const bool block = fb && prefix_blocked(ev, my_rank, ord + env_of_lane * A, woff + env_of_lane * A, any_writes,
                                                                (m_moved & genv) >> (env_of_lane * A), A);
                        wave_sync();
                        if (block) ord[env_of_lane * A + my_rank] = (uint8_t)(agent_of_lane | 0x40);
                        wave_sync();
                        bool prefix_ok = fb;
                        if (fb)
                            for (int k = 0; k < my_rank; ++k) prefix_ok &= (ord[env_of_lane * A + k] & 0x40) == 0;
                        prefix_ok = prefix_ok && !block;
                        wave_sync();
                        if (in) ord[env_of_lane * A + my_rank] = (uint8_t)(agent_of_lane | (prefix_ok ? 0x80 : 0));   // (bit 7: "this turn is done")
                        does_act = does_act || prefix_ok;
                    }
                }
                if (!PREFIX || A <= 2) {
                    const bool first_ok = fb && my_rank == 0 && !(ev.bad | ev.success | ev.failure);
                    if (first_ok) ord[env_of_lane * A] = (uint8_t)(agent_of_lane | 0x80);
                    does_act = does_act || first_ok;
                }
            }
        }
        if (does_act) {                                                              // commit
            if (ev.go) { rows[lane] = ev.nrow; cur_row = ev.nrow; }
            if (ev.unstale) reinterpret_cast<uint8_t *>(auxl + env_of_lane)[4] = 0;
            if (ev.writes) {
                store_cell(CB, mytile + ev.off, ev.ncell);
                if (!ROLL) {                                                     // ROLL writes the whole tile back at the end
                    if constexpr (B3) store_obs_cell(MGX_LATE(grid) + (e0 + env_of_lane) * (int64_t)HWG + (ev.off >> 1) * 3, ev.ncell);
                    else store_cell(CB, MGX_LATE(grid) + (e0 + env_of_lane) * HWB + ev.off, ev.ncell);
                    if constexpr (MARK) {                                        // the env has left its pool layout
                        int32_t *const p_lay = MGX_LATE(grid_layout);
                        if (p_lay) p_lay[e0 + env_of_lane] = -1;
                    }
                }
            }
        }
        if (m_evt != 0) {                                                        // on_success / on_failure of the agents that acted
            const uint64_t m_succ = __builtin_amdgcn_ballot_w64(does_act && ev.success);
            if (in && !fb) {
                if (cf.joint_reward ? (m_succ & genv) != 0 : (does_act && ev.success))
                    my_rew = reward_value(scnt[env_of_lane] + 1, cf.max_steps);          // base.py:500-507, 598-602
                if ((does_act && event_ends_self(cf, ev)) || (m_ends & genv) != 0) {          // base.py:478-498, 509-532
                    cur_row |= 1ull << 32;
                    rows[lane] = cur_row;
                }
            }
        }
        MGX_MARK("P1s_end");
        const uint64_t fbw = __builtin_amdgcn_ballot_w64(fb);                   // envs that need the sequential loop
        MGX_SPAN_FLAG(2, fbw != 0);
        MGX_SPAN_FLAG(4, m_evt != 0);
        wave_sync();
        if (fbw != 0) {
            // (P1b, the argsort by ranking of base.py:399, has been done where the fallback was decided: `ord` holds it)
            // -------------------------------------------------------------- P1c: one lane per env: the reference's loop
            const bool mine = lane < Gc && (lane * A < 64) && ((fbw >> (lane * A)) & 1ull);
            if (mine) {
                const int e = lane;
                const int64_t b = e0 + e;
                uint8_t *etile = tile + e * TSB;
                uint8_t *ggrid = MGX_LATE(grid) + b * HWG;
                [[maybe_unused]] int32_t *const p_lay = MARK ? MGX_LATE(grid_layout) : nullptr;
                auto dirty = [=](int off) {
                    if constexpr (B3) store_obs_cell(ggrid + (off >> 1) * 3, cell_unpack_full(load_cell16(etile + off)));
                    else if (!ROLL) store_cell_raw(CB, ggrid + off, load_cell_raw(CB, etile + off));
                    if constexpr (MARK) { if (p_lay) p_lay[b] = -1; }            // (the layout marker: this env has left its pool layout)
                };
                int k0 = 0;                                                     // the agents below the cutoff have committed already
                if constexpr (PREFIX) { if (A > 1) while (k0 < A && (ord[e * A + k0] & 0x80)) ++k0; }
                else k0 = (A > 1 && (ord[e * A] & 0x80)) ? 1 : 0;
                const int rc = handle_actions(cf, etile, rows + e * A, acts + e * A, ord + e * A, rew + e * A,
                                              scnt[e] + 1, dirty, reinterpret_cast<uint8_t *>(auxl + e), env_kind, k0);
                int32_t *errp = MGX_LATE(err);
                if (rc != 0 && errp) { atomicAdd(errp, 1); atomicMin(errp + 1, (int32_t)min(b, (int64_t)INT_MAX)); }
            }
            wave_sync();
        }
        MGX_MARK("P1hook");
        // ------------------------------------------------------------------ overlay offsets (pre-hook `terminated`, SURVEY
        // App. C Q2), then one lane per env: counters + the env subclass' hook on the clean tile, then the overlay itself
        const int ovl = (in && !MGX_DBG(512)) ? overlay_offset(cf, rows + env_of_lane * A, agent_of_lane) : -1;
        if (HOOKS && in && !fb) rew[lane] = my_rew;                              // (the hooks assign to / add onto the base rewards)
        // the hooks' visiting order goes where the (by now dead) action visiting order lay
        const uint8_t *const p_hord = HOOKS ? MGX_LATE(hook_order) : nullptr;
        if (HOOKS && p_hord && in) ord[lane] = ROLL ? p_hord[tv0 + lane] : in_hord;
        wave_sync();
        if (lane < Gc) {
            const int e = lane;
            const int64_t b = e0 + e;
            const int32_t sc = (ROLL ? scnt[e] : (int32_t)in_scnt) + 1;          // base.py:333
            if (ROLL) scnt[e] = sc; else p_step_count[b] = sc;
            uint8_t *etile = tile + e * TSB;
            uint8_t *ggrid = MGX_LATE(grid) + b * HWG;
            auto dirty = [=](int off) {
                if constexpr (B3) store_obs_cell(ggrid + (off >> 1) * 3, cell_unpack_full(load_cell16(etile + off)));
                else if (!ROLL) store_cell_raw(CB, ggrid + off, load_cell_raw(CB, etile + off));
                if constexpr (MARK) {                                            // (the layout marker: as in P1c.  No hook writes a cell
                    int32_t *const p_lay = MGX_LATE(grid_layout);                // today: the load is only made where one does)
                    if (p_lay) p_lay[b] = -1;
                }
            };
            uint8_t *eaux = reinterpret_cast<uint8_t *>(auxl + e);
            post_step_hook(cf, env_kind, etile, rows + e * A, acts + e * A, eaux, sc, rew + e * A, dirty, p_hord ? ord + e * A : nullptr);
            if (!ROLL && cv.has_aux) {                                           // the hook state the step may change
                uint8_t *gaux = MGX_LATE(aux) + b * MGX_AUX_BYTES;
                if (env_kind == MGX_KIND_LOCKEDHALLWAY) { gaux[1] = eaux[1]; gaux[2] = eaux[2]; gaux[15] = eaux[15]; }
                if (env_kind == MGX_KIND_REDBLUEDOORS) gaux[4] = eaux[4];
            }
            MGX_PUB_STORE_U8(p_truncated + tb0 + e0, e, Gc, sc >= cf.max_steps);                     // base.py:339
        }
        wave_sync();
        if ((HOOKS || fbw != 0) && in) {                                         // (a hook / the fallback may have terminated it
            cur_row = rows[lane];                                                // and rewarded it: their results are in LDS)
            if (HOOKS || fb) my_rew = rew[lane];
        }
        if (ROLL && ovl >= 0) ovl_saved = load_cell_raw(CB, mytile + ovl);
        ovl_off = ovl;
        wave_sync();
        if (ovl >= 0) {
            MGX_CHECK_LDS_PTR(3, mytile + ovl, CB);
            store_cell_raw(CB, mytile + ovl, agent_cell_raw(CB, cur_row));
        }
    } else {
        const int off = (lane < NVc) ? overlay_offset(cf, rows + env_of_lane * A, agent_of_lane) : -1;
        wave_sync();
        if (off >= 0) store_cell_raw(CB, tile + env_of_lane * TSB + off, agent_cell_raw(CB, cur_row));
    }
    wave_sync();

    MGX_MARK("P1d");
    // ------------------------------------------------------------------ P1d: one lane per view: geometry + outputs
    const uint32_t tile_addr = (uint32_t)(wave * wave_lds_ + cv.tile(sl_s) + tile_skew);   // LDS address of env 0 cell 0
    uint32_t my_carry = 0;                                                   // slot `lane`: what its agent carries
    // (the output pointers are fetched first so that the s_load latency hides behind the geometry arithmetic)
    uint8_t *const p_dir = MGX_LATE(dir);
    uint8_t *const p_agents = DO_STEP ? MGX_LATE(agents) : nullptr;
    double *const p_reward = DO_STEP ? MGX_LATE(reward) : nullptr;
    uint8_t *const p_term = DO_STEP ? MGX_LATE(terminated) : nullptr;
    if (lane < NVc) {
        const int e = env_of_lane;
        const uint64_t row = cur_row;
        const ViewGeom g = view_geom<V>(W, H, row_x(row), row_y(row), row_dir(row), CB, PITCH);
        const ViewClamp vc = view_clamp<V>(g, W, H, row_x(row), row_y(row));
        ViewRec r;                                                             // (an agent outside the grid sees only walls)
        r.origin = vc.valid ? (int32_t)tile_addr + e * TSB + g.origin : (int32_t)wall_addr;
        r.steps = vc.valid ? vc.steps : 0u; r.lo = vc.valid ? vc.lo : 0u; r.hi = vc.valid ? vc.hi : 0u;
        my_carry = row_carry(row) & kCellShown;                               // (a carried box shows as a box, whatever it holds)
        rec[lane] = r;
        if (DO_STEP) {
            const u32x2 rowv = {(uint32_t)row, (uint32_t)(row >> 32)};
            if (!ROLL) __builtin_amdgcn_raw_buffer_store_b64(rowv, make_rsrc(p_agents + v0 * 8, NVc * 8), lane * 8, 0, kSmallOutAux);
            const uint64_t rbits = __builtin_bit_cast(uint64_t, my_rew);
            const u32x2 rewv = {(uint32_t)rbits, (uint32_t)(rbits >> 32)};
            __builtin_amdgcn_raw_buffer_store_b64(rewv, make_rsrc(p_reward + tv0, NVc * 8), lane * 8, 0, kOutAux);
            const bool forced = env_kind == MGX_KIND_LOCKEDHALLWAY && reinterpret_cast<const uint8_t *>(auxl + e)[15];
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(row_term(row) | forced),                    // base.py:338 (+ env hook)
                                                 make_rsrc(p_term + tv0, NVc), lane, 0, kOutAux);
        }
        if (p_dir) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)row_dir(row), make_rsrc(p_dir + tv0, NVc), lane, 0, kOutAux);   // base.py:359, 372
    } else if (lane < ((NVc + kG - 1) & ~(kG - 1))) {                // padding slots of the last gather group
        ViewRec r;
        r.origin = (int32_t)wall_addr; r.steps = 0; r.lo = 0; r.hi = 0;
        rec[lane] = r;
    }
    wave_sync();

    // GEN with candidates (include/mgx.h: MgxGenStage.candidates): the step's rules have run -- an env whose episode ENDS with this
    // step (by truncation or by an event alike) draws the door row from np_random as this step left it and asks for that candidate
    // NOW: the slot arrives under P2..P5 and is stored in the tail (the first such env of the wavefront; others load in the tail)
    if constexpr (GEN && MODE == 1) {
        // the envs whose episode ENDS with this step (base.py:534-539 on the post-step state): known as soon as the rules have run.
        // Tested HERE, not in the tail: a wavefront without one -- nearly all of them -- then leaves through one scalar branch
        // (from registers: every agent's lane holds its final row, the env's lane its step count -- one ballot instead of A LDS reads)
        const uint64_t alive_now = __builtin_amdgcn_ballot_w64(lane < NVc && !row_term(cur_row));     // bit = (env, agent) slot
        if (lane < Gc) {
            const uint64_t amask = (A >= 64) ? ~0ull : ((1ull << A) - 1ull);
            done_now = (((alive_now >> mad24(lane, A, 0)) & amask) == 0) | ((int32_t)in_scnt + 1 >= cf.max_steps);
            uint8_t *wr = MGX_LATE(was_reset);
            if (wr) wr[e0 + lane] = (uint8_t)done_now;
        }
        done_mask = __builtin_amdgcn_ballot_w64(done_now);
        if (stage_tag && cand_K > 0) {
            const bool dn = done_now;
            if (done_mask != 0) {                                                    // rare
                cand_r = cand_draw(cand_npr);
                const int r = cand_r;
                const int32_t tr = (int32_t)(r == 0 ? in_tags.x : r == 1 ? in_tags.y : r == 2 ? in_tags.z : in_tags.w);
                cand_mask = __builtin_amdgcn_ballot_w64(dn && tr == (int32_t)in_ep);
                if (cand_mask != 0 && (HWB & 3) == 0 && HWB <= 1024) {
                    pre_e = __builtin_ctzll(cand_mask);
                    const int64_t s = (e0 + pre_e) * cand_K + __builtin_amdgcn_readlane(r, pre_e);
                    const uint32_t *sg = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(MGX_LATE_STAGE(grid)) + s * HWB);
                    const int nd = HWB / 4;
#pragma unroll
                    for (int k = 0; k < 4; ++k) pre_grid[k] = (lane + 64 * k < nd) ? sg[lane + 64 * k] : 0u;
                    pre_row = lane < A ? (reinterpret_cast<const uint64_t *>(MGX_LATE_STAGE(agents)) + s * A)[lane] : 0ull;
                    pre_word = lane < 5 ? (MGX_LATE_STAGE(words) + s * 6)[lane] : 0ull;
                    if (HOOKS) pre_aux = reinterpret_cast<const uint4 *>(MGX_LATE_STAGE(aux))[s];
                }
            }
        }
    }

    MGX_MARK("P2");
    // ------------------------------------------------------------------ P2: the wavefront renders its views, one lane per cell
    const LaneConst<V, NW> lc = ROLL ? lc_roll : lane_consts();
    uint32_t cell[HALF ? VPW / 2 : VPW][NW];     // registers: every slot's packed cells, one per lane (and pass); HALF: slots 2p
                                                 // and 2p+1 in the halves of one register; P4 reads only the gathered ones (s < NVc)
    uint32_t sbLo[NW], sbHi[NW];                 // lane s holds the see-behind ballot of slot s
#pragma unroll
    for (int k = 0; k < NW; ++k) { sbLo[k] = 0; sbHi[k] = 0; }
    // LINES: a lane's V cells of its line, two per register, for every pass of 8 slots; the lines' see-behind bytes [slot][line], then
    // in place the visibility bytes, over the packed agent rows (dead: a one-step kernel has them in registers from P1d on)
    [[maybe_unused]] uint32_t cellp[LINES ? VPW / kLineLanes : 1][(V + 1) / 2];
    [[maybe_unused]] uint8_t *const line_bytes = L + cv.rows();
    if constexpr (LINES) {
        static_assert(!ROLL && !SLICED && NW == 1 && VPW % kGroup == 0, "line map: one-step kernels, views of one lane pass");
        if (!MGX_DBG(4)) gather_lines<V, VPW, 0>(a, wave, lane, NVc, rec, line_bytes, cellp);
    } else
    if (!MGX_DBG(4)) gather_all<V, NW, VPW, HALF, kG, C8>(a, wave, NVc, rec, lc, cell, sbLo, sbHi,
                                                          (uint32_t)(wave * wave_lds_ + cv.lut() + 512));
    if (ROLL) {                                                              // take the overlay off again: the tile persists
        wave_sync();
        if (ovl_off >= 0) store_cell_raw(CB, tile + env_of_lane * TSB + ovl_off, ovl_saved);
    }

    MGX_MARK("P3");
    // ------------------------------------------------------------------ P3: lane s floods the visibility of slot s
    const bool masked = !a.sp.see_through_walls;                                // obs.py:95-100
    uint32_t visLo[NW], visHi[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) { visLo[k] = 0xffffffffu; visHi[k] = 0xffffffffu; }
    if constexpr (LINES) {
        // lane s: the 8 see-behind bytes of slot s as one word (rows 8 bits apart), flooded, written back as its visibility bytes
        wave_sync();
        if (lane < NVc) {
            u32x2 *const w = reinterpret_cast<u32x2 *>(line_bytes) + lane;
            MGX_CHECK_LDS_PTR(13, w, 8);
            uint64_t vis = ~0ull;
            if (masked && !MGX_DBG(8)) {
                const u32x2 sbw = *w;
                // (the bytes hold the cells' OPAQUE bits: see-behind is their complement)
                const uint64_t sb = (~(((uint64_t)sbw.y << 32) | sbw.x) & ~(1ull << kLineOwnBit<V>))     // own cell: what it carries
                                  | ((uint64_t)see_behind(my_carry) << kLineOwnBit<V>);
                vis = vis_mask_lines<V>(sb);
            }
            *w = u32x2{(uint32_t)vis, (uint32_t)(vis >> 32)};
        }
        wave_sync();
    } else
    if (masked && !MGX_DBG(8)) {
        uint64_t sb[NW], vis[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) sb[k] = ((uint64_t)sbHi[k] << 32) | sbLo[k];
        constexpr int kOwn = (V - 1) * V + V / 2;                               // the agent's own cell: image[V/2][V-1]
        sb[kOwn >> 6] = (sb[kOwn >> 6] & ~(1ull << (kOwn & 63)))              // ... shows what it carries (obs.py:207)
                      | ((uint64_t)see_behind(my_carry) << (kOwn & 63));
        vis_mask<V, NW>(sb, vis);
#pragma unroll
        for (int k = 0; k < NW; ++k) { visLo[k] = (uint32_t)vis[k]; visHi[k] = (uint32_t)(vis[k] >> 32); }
    }

    MGX_MARK("P4");
    // slot s's packed cell in this lane (HALF: bits 16.. of an even slot's value are the odd slot's cell -- cell_unpack's masks
    // drop them)
    auto slot_cell = [&](const int s, const int it) -> uint32_t {
        if constexpr (HALF) return (s & 1) ? cell[s >> 1][it] >> 16 : cell[s >> 1][it];
        else return cell[s][it];
    };
    // (compact cells: the gathered value is the decode table's entry: already (type, color, state))
    auto to_obs = [](const uint32_t c) -> uint32_t { if constexpr (C8) return c; else return cell_unpack(c); };
    if constexpr (OH) {
        // -------------------------------------------------------------- P4'/P5' (one-hot output) in rounds of kR slots:
        // P4' masks each cell and leaves its one-hot bit mask (bit t | bit 11+c | bit 17+s) at its image position in LDS;
        // P5' turns the masks of the 1-2 cells that each run of 16 output bytes spans into 0/1 bytes and streams them out.
        constexpr int D = 21;
        constexpr uint32_t kInvD = 0xFFFFFFFFu / D + 1u;                        // ceil(2^32 / 21): x / 21 exact for x < 2^20
        const int64_t h0 = tv0 * (int64_t)(V2 * D), h1 = h0 + (int64_t)NVc * V2 * D;
        const int oh_skew = (int)(h0 & 15);
        uint32_t *masks = reinterpret_cast<uint32_t *>(L + cv.out()) + 1;      // masks[-1] and masks[cells] are readable pads
        auto one_hot_mask = [](uint32_t c) -> uint32_t { return one_hot_mask21(c); };   // out-of-range values set no bit (as mgx_one_hot)
        // (compact cells: the registers hold the decode table's entries, which ARE the masks -- an unseen cell takes UNSEEN's)
        constexpr uint32_t kUnseenMask = 1u | (1u << 11) | (1u << 17);
        auto cell_mask = [&](const bool seen, const uint32_t x) -> uint32_t {
            if constexpr (C8) return seen ? x : kUnseenMask;
            else return one_hot_mask(to_obs(seen ? x : CELL_UNSEEN));
        };
        if (lane == 0) masks[-1] = 0;
#pragma unroll
        for (int r0 = 0; r0 < VPW; r0 += kR) {
            if (r0 < NVc) {
#pragma unroll
                for (int it = 0; it < NW; ++it) {
                    if (lc.act[it]) {
                        uint32_t *d0 = masks + (lc.q3[it] / 3);                  // q3 = 3 * (i*V + j)
                        if constexpr (PK3) {
                            if (it == 1) {                                       // the shared remainder passes (see P4 below)
                                constexpr int R = V2 - 64, NP = pack3_passes(kG), kLast = kG - 3 * (NP - 1);
#pragma unroll
                                for (int g0 = 0; g0 < kR; g0 += kG) {
                                    if (r0 + g0 < NVc) {
#pragma unroll
                                        for (int p = 0; p < NP; ++p) {
                                            const int ns = p == NP - 1 ? kLast : 3, sl = g0 + 3 * p, s = r0 + sl;
                                            uint64_t m = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visLo[1], s);
                                            if (ns > 1) m |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visLo[1], s + 1) << R;
                                            if (ns > 2) m |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visLo[1], s + 2) << (2 * R);
                                            const uint32_t x = C8 ? cell[pk3_reg<kG>(r0 + g0, p)][1] : (cell[pk3_reg<kG>(r0 + g0, p)][1] & 0xffffu);
                                            if (ns == 3 || lane < ns * R) {
                                                MGX_CHECK_LDS_PTR(7, d0 + sl * V2, 4);
                                                d0[sl * V2] = cell_mask(__builtin_amdgcn_inverse_ballot_w64(m), x);
                                            }
                                        }
                                    }
                                }
                                continue;
                            }
                        }
#pragma unroll
                        for (int g0 = 0; g0 < kR; g0 += kG) {
                            if (r0 + g0 < NVc) {
#pragma unroll
                                for (int sl = g0; sl < g0 + kG; ++sl) {
                                    const int s = r0 + sl;
                                    // (a pass of at most 32 cells has no high word)
                                    const uint64_t m = (V2 - 64 * it > 32 ? (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visHi[it], s) << 32 : 0ull)
                                                     | (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visLo[it], s);
                                    MGX_CHECK_LDS_PTR(7, d0 + sl * V2, 4);
                                    d0[sl * V2] = cell_mask(__builtin_amdgcn_inverse_ballot_w64(m), slot_cell(s, it));
                                }
                            }
                        }
                    }
                }
                wave_sync();
                if (lane >= r0 && lane < r0 + kR && lane < NVc)             // own cell := carried object (obs.py:207)
                    masks[(lane - r0) * V2 + (V / 2) * V + (V - 1)] = one_hot_mask(my_carry);
                wave_sync();
                MGX_MARK("P5");
                const int64_t ro0 = h0 + (int64_t)r0 * (V2 * D);                // this round's output bytes [ro0, ro1)
                const int rbytes = (int)min((int64_t)kR * V2 * D, h1 - ro0);
                const int rlen = oh_skew + rbytes;                              // from the aligned start
                uint8_t *gdst = MGX_LATE(obs) + (ro0 - oh_skew);
                const __amdgpu_buffer_rsrc_t orsrc = make_rsrc(gdst, rlen);
                for (int rel = lane16; rel < rlen; rel += 1024) {
                    // output bytes [rel, rel + 16) of the aligned run = round bytes x .. x + 15, x = rel - skew (may be < 0:
                    // shifted by one cell so that the division stays in the positives; masks[-1] is a pad)
                    const uint32_t xs = (uint32_t)(rel - oh_skew + D);
                    const uint32_t cq = __umulhi(xs, kInvD);                    // cell + 1
                    const uint32_t k0 = xs - cq * D;                            // first bit inside that cell: 0..20
                    MGX_CHECK_LDS_PTR(8, masks + (int)cq - 1, 8);
                    const uint32_t bits = (masks[(int)cq - 1] >> k0) | (masks[(int)cq] << (D - k0));   // >= 22 valid bits
                    u32x4 v;
                    v.x = (((bits >> 0) & 0xfu) * 0x00204081u) & 0x01010101u;   // 4 bits -> 4 bytes of 0/1
                    v.y = (((bits >> 4) & 0xfu) * 0x00204081u) & 0x01010101u;
                    v.z = (((bits >> 8) & 0xfu) * 0x00204081u) & 0x01010101u;
                    v.w = (((bits >> 12) & 0xfu) * 0x00204081u) & 0x01010101u;
                    if ((rel + 16 <= rlen) & (rel >= oh_skew)) {
                        __builtin_amdgcn_raw_buffer_store_b128(v, orsrc, rel, 0, PERSIST ? 16 : kOhAux);
                    } else {                                                    // ragged head / tail of the wave's bytes
                        const int lo_b = max(rel, oh_skew), hi_b = min(rel + 16, rlen);
#pragma clang loop vectorize(disable) unroll(disable)
                        for (int B = lo_b; B < hi_b; ++B) {                     // (selects, not an indexed array: no stack object)
                            const int q = (B - rel) >> 2;
                            const uint32_t w = q == 0 ? v.x : (q == 1 ? v.y : (q == 2 ? v.z : v.w));
                            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(w >> (8 * ((B - rel) & 3))), orsrc, B, 0, PERSIST ? 16 : 0);
                        }
                    }
                }
                wave_sync();
                MGX_MARK("P5end");
            }
        }
    } else {
    [[maybe_unused]] const int64_t o0 = tv0 * (int64_t)(V2 * 3), o1 = o0 + (int64_t)NVc * V2 * 3;  // this wave's obs bytes (of step t)
    if constexpr (obs_dword_staging(V, ROLL)) {
    // ------------------------------------------------------------------ P4/P5 in rounds of kR slots, one dword per cell (round 7):
    // P4 masks each cell and stores it as ONE dword (type, color, state, junk) at its image position in LDS -- the same address
    // every round, its slot in the store's immediate offset; P5 reads 4 cells per lane (ds_read_b128), packs them into 12 bytes
    // (mgx_rules.h obs_unit: 3 v_perm_b32, 3 more when the wave's bytes do not start on a dword) and stores them with one
    // buffer_store_dwordx3.  The 3-byte staging it replaces took two LDS stores per cell (ds_write_b16 + ds_write_b8_d16_hi: a
    // view is an odd number of bytes, so every other cell starts at an odd address), ~8.8 LDS-pipe cycles against 4 now.
    // (ds_write_addtid_b32 would store in 2 cycles, but at lane order: lane k holds image cell k = j*V + i, the observation's
    // order is i*V + j, so P5 would gather 4-5 scattered dwords per lane from per-lane addresses instead of one ds_read_b128.)
    static_assert(NW == 1 && !PK3 && !PERSIST && kR % 4 == 0, "dword staging: views of one lane pass, rounds of whole dwords");
    uint32_t *const stg = reinterpret_cast<uint32_t *>(L + cv.out()) + 4;     // cell c of the round at stg[c]; stg[-4..-1]: pad
    const int s_w = (int)(o0 & 3);                                              // the wave's first obs byte, within its dword
    // ONE buffer resource for the wave: its bytes from the dword they start in; a round's offset goes into soffset
    const __amdgpu_buffer_rsrc_t orsrc = make_rsrc(MGX_LATE(obs) + (o0 - s_w), s_w + NVc * V2 * 3);
    constexpr int kUnits = kR * V2 / 4 + 1;                                     // 12-byte units of a round (+1: its ragged tail)
    constexpr int kPasses = (kUnits + 63) / 64;
    uint32_t *const d0 = stg + lc.q3[0] / 3;                                    // this lane's cell: image[i][j] = cell i*V + j
    // P5 of a WHOLE round of a wave whose bytes start on a dword -- every round of C4, C2, C3 and C4's 8192-env share: its kR*V*V/4
    // units are all whole, so no lane needs a bound or the ragged path, and the round's reads are all issued before the first use
    auto p5_whole = [&](const int r0) {
        constexpr int kWhole = kR * V2 / 4, kWP = (kWhole + 63) / 64;
        u32x4 d[kWP];
#pragma unroll
        for (int k = 0; k < kWP; ++k) {                                         // (the last pass's idle lanes read the last unit)
            const int u = 64 * (k + 1) <= kWhole ? lane + 64 * k : min(lane + 64 * k, kWhole - 1);
            MGX_CHECK_LDS_PTR(6, stg + 4 * u, 16);
            d[k] = *reinterpret_cast<const u32x4 *>(stg + 4 * u);
        }
#pragma unroll
        for (int k = 0; k < kWP; ++k) {
            uint32_t w[3];
            obs_unit(0u, d[k].x, d[k].y, d[k].z, d[k].w, 0, w);
            if (64 * (k + 1) <= kWhole || lane + 64 * k < kWhole)
                __builtin_amdgcn_raw_buffer_store_b96(u32x3{w[0], w[1], w[2]}, orsrc, 12 * (lane + 64 * k), r0 * V2 * 3,
                                                      kObsAux);
        }
    };
    // P5 of any round at r0 (a wave's last, partial one; a wave whose bytes start s = s_w bytes into a dword)
    auto p5_round = [&](const int r0, const int s) {
        const int roff = r0 * V2 * 3;                                           // the round's bytes, from the wave's first
        const int ulen = s + (int)min(kR * V2 * 3, (NVc - r0) * V2 * 3);        // ... and its window of whole dwords
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            const int u = lane + 64 * k, ub = 12 * u;                          // unit u: window bytes [12u, 12u + 12)
            if (ub < ulen) {
                MGX_CHECK_LDS_PTR(6, stg + 4 * u - 1, 20);
                const u32x4 d = *reinterpret_cast<const u32x4 *>(stg + 4 * u);  // cells 4u .. 4u + 3
                const uint32_t dm1 = s ? stg[4 * u - 1] : 0u;                   // cell 4u - 1
                uint32_t w[3];
                obs_unit(dm1, d.x, d.y, d.z, d.w, s, w);
                if (ub >= s && ub + 12 <= ulen) {
                    __builtin_amdgcn_raw_buffer_store_b96(u32x3{w[0], w[1], w[2]}, orsrc, ub, roff, kObsAux);
                } else {                                                        // the ragged head / tail of the round's bytes
                    const int lo_b = max(s - ub, 0), hi_b = min(ulen - ub, 12);
#pragma clang loop vectorize(disable) unroll(disable)
                    for (int B = lo_b; B < hi_b; ++B) {                         // (selects, not an indexed array: no stack object)
                        const uint32_t x = B < 4 ? w[0] : (B < 8 ? w[1] : w[2]);
                        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(x >> (8 * (B & 3))), orsrc, ub + B, roff, 0);
                    }
                }
            }
        }
    };
    // LINES: lane (slot, j)'s visibility byte of every pass, all read before the first round's staging stores
    [[maybe_unused]] uint32_t line_vis[LINES ? VPW / kLineLanes : 1];
    if constexpr (LINES) {
#pragma unroll
        for (int p = 0; p < VPW / kLineLanes; ++p) {
            line_vis[p] = 0;
            if (p * kLineLanes / kR * kR < NVc) {
                MGX_CHECK_LDS_PTR(14, line_bytes + p * 64 + lane, 1);
                line_vis[p] = line_bytes[p * 64 + lane];
            }
        }
    }
#pragma unroll
    for (int r0 = 0; r0 < VPW; r0 += kR) {
        if (r0 < NVc) {
            if (!MGX_DBG(16)) {
                if constexpr (LINES) {
                    // lane (slot, j) masks and unpacks the V cells of its line and stores them at image[i][j] = cell i*V + j of its
                    // slot: the round's two passes of 8 slots, straight-line (whole groups; padding slots write junk that P5 never copies)
                    constexpr int PR = kR / kLineLanes;
                    const int lj = lane & (kLineLanes - 1);
                    if (lj < V) {
                        uint32_t *const dl = stg + (lane >> 3) * V2 + lj;
#pragma unroll
                        for (int q = 0; q < PR; ++q) {
                            const uint32_t vb = line_vis[r0 / kLineLanes + q];
#pragma unroll
                            for (int k = 0; k < (V + 1) / 2; ++k) {
                                const uint32_t x = cellp[r0 / kLineLanes + q][k];
                                const uint32_t tc = x & 0x070f070fu, st = (x >> 12) & 0x00030003u;
#pragma unroll
                                for (int i = 2 * k; i < 2 * k + 2 && i < V; ++i) {
                                    MGX_CHECK_LDS_PTR(5, dl + q * kLineLanes * V2 + i * V, 4);
                                    dl[q * kLineLanes * V2 + i * V] = line_stage_cell(tc, st, i, vb);
                                }
                            }
                        }
                    }
                } else
                if (lc.act[0]) {
                    // whole groups of kG slots, like P2 (padding slots write junk into staging space that P5 never copies):
                    // straight-line code whose readlane -> select -> write chains overlap
#pragma unroll
                    for (int g0 = 0; g0 < kR; g0 += kG4) {
                        if (r0 + g0 < NVc) {
#pragma unroll
                            for (int sl = g0; sl < g0 + kG4; ++sl) {
                                const int s = r0 + sl;
                                // (see_through_walls: the masks are all ones -- no branch, it would fence the schedule)
                                // (a pass of at most 32 cells has no high word)
                                const uint64_t m = (V2 > 32 ? (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visHi[0], s) << 32 : 0ull)
                                                 | (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visLo[0], s);
                                // packed cell(s) -> (type, color, state) in bytes 0-2 (cell_unpack's fields; the pair's two ANDs
                                // and the shift are common to both of its slots); compact cells: the decoded entry already is
                                const uint32_t x = HALF ? cell[s >> 1][0] : cell[s][0];
                                const uint32_t c = C8 ? x : perm_b32((x >> 12) & 0x00030003u, x & 0x070f070fu, obs_stage_sel(HALF && (s & 1)));
                                MGX_CHECK_LDS_PTR(5, d0 + sl * V2, 4);
                                d0[sl * V2] = __builtin_amdgcn_inverse_ballot_w64(m) ? c : 0u;   // UNSEEN = (0, 0, 0)
                            }
                        }
                    }
                }
                wave_sync();
                // lane r0+sl: its agent's own cell shows the carried object (obs.py:207; always visible, obs.py:252)
                if (lane >= r0 && lane < r0 + kR && lane < NVc) {
                    MGX_CHECK_LDS_PTR(5, stg + (lane - r0) * V2 + (V / 2) * V + (V - 1), 4);
                    stg[(lane - r0) * V2 + (V / 2) * V + (V - 1)] = my_carry;
                }
            }
            wave_sync();
            MGX_MARK("P5");
            if (!MGX_DBG(32)) {
                if (s_w == 0 && r0 + kR <= NVc) p5_whole(r0);
                else p5_round(r0, s_w);
            }
            wave_sync();
            MGX_MARK("P5end");
        }
    }
    } else {
    // ------------------------------------------------------------------ P4/P5 in rounds of kR slots, the observation's 3-byte cells
    // (the rollout / persistent kernels, whose staging may lie over the view records, and views of more than one lane pass):
    // P4 masks each cell and transposes it into the obs byte layout in LDS, P5 streams the round to HBM in 16-byte vectors
    // (round 6 tried software-pipelined rounds -- the next round's P4 arithmetic under this round's staging reads: 5-6 % slower at
    // C4, profiles/r6_p45_pipeline_ab.txt)
    const int out_skew0 = (int)(o0 & 15);                                       // the same for every round (rounds of 16 slots are
    uint8_t *out_raw = L + cv.out();                                          // whole 16-byte vectors; the sliced kernels' rounds of 8
    constexpr int kRoundBytes = kR * V2 * 3;                                // slots alternate by 8 bytes)
#pragma unroll
    for (int r0 = 0; r0 < VPW; r0 += kR) {
        const int out_skew = (kRoundBytes & 15) ? ((out_skew0 + ((r0 * V2 * 3) & 15)) & 15) : out_skew0;
        uint8_t *const outb = out_raw + out_skew;                             // obs bytes [oa_r, ...) of round r
        if (r0 < NVc) {
            if (!MGX_DBG(16)) {
#pragma unroll
                for (int it = 0; it < NW; ++it) {
                    if (lc.act[it]) {
                        uint8_t *d0 = outb + lc.q3[it];
                        // A cell's 3 bytes go out as one ALIGNED 2-byte store + one byte store (an LDS store costs the same
                        // VGPR -> LDS transfer whatever its width, so 2 stores instead of 3).  A view is an odd number of
                        // bytes, so the parity of a cell's first byte alternates from slot to slot: even slots use [0], odd [1].
                        const uint32_t par0 = (uint32_t)(out_skew + lc.q3[it]) & 1u;
                        uint8_t *const d16[2] = {d0 + par0, d0 + (par0 ^ 1u)};                  // the 2-byte part: bytes 0-1 or 1-2
                        uint8_t *const d8[2] = {d0 + 2u * (par0 ^ 1u), d0 + 2u * par0};         // the other byte: 2 or 0
                        // (round 3) ONE v_perm_b32 per slot makes the register both stores read -- bytes 0-1 = the 2-byte part,
                        // byte 2 = the other byte (ds_write_b16 / ds_write_b8_d16_hi): no widening chain, no per-store shifts.
                        // Its sources are made once per PAIR of slots sharing a cell register (HALF; per slot otherwise):
                        // tc = (type, color) bytes of both halves, st = the state in byte 0 of both halves.  Selector bytes: 0-3 =
                        // tc bytes, 4-7 = st bytes, 0x0c = 0x00.  [0]: the slot in the register's low half, [1]: high half (HALF) /
                        // odd slots; the parity of the cell's first output byte is par0 for [0] and the opposite for [1].
                        //   first byte even: (type, color | state)    first byte odd: (color, state | type)
                        // (compact cells: the register already holds (type, color, state) in bytes 0-2: first byte even = as it is,
                        // odd = rotated by one byte)
                        const uint32_t sel[2] = {C8 ? (par0 ? 0x0c000201u : 0x0c020100u) : (par0 ? 0x0c000401u : 0x0c040100u),
                                                 C8 ? (par0 ? 0x0c020100u : 0x0c000201u)
                                                    : (HALF ? (par0 ? 0x0c060302u : 0x0c020603u) : (par0 ? 0x0c040100u : 0x0c000401u))};
                        if constexpr (PK3) {
                            if (it == 1) {
                                // the shared remainder passes (mgx_fused.h: kPack3): pass p of a group holds cell 64 + lane % R of
                                // the views g0 + 3p + lane / R; its lane predicate = the three views' R-bit visibility words side
                                // by side (scalar shifts); q3[1] carries the lane's view offset, so the staging address and the
                                // parity of its first byte follow from the pass's FIRST view exactly as for a whole view
                                constexpr int R = V2 - 64, NP = pack3_passes(kG), kLast = kG - 3 * (NP - 1);
                                const uint32_t selR[2] = {C8 ? sel[0] : (par0 ? 0x0c000401u : 0x0c040100u),
                                                          C8 ? sel[1] : (par0 ? 0x0c040100u : 0x0c000401u)};
#pragma unroll
                                for (int g0 = 0; g0 < kR; g0 += kG) {
                                    if (r0 + g0 < NVc) {
#pragma unroll
                                        for (int p = 0; p < NP; ++p) {
                                            const int ns = p == NP - 1 ? kLast : 3, sl = g0 + 3 * p, s = r0 + sl;
                                            uint64_t m = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visLo[1], s);
                                            if (ns > 1) m |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visLo[1], s + 1) << R;
                                            if (ns > 2) m |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visLo[1], s + 2) << (2 * R);
                                            const uint32_t x = cell[pk3_reg<kG>(r0 + g0, p)][1];
                                            const uint32_t tc = C8 ? x : (x & 0x070fu), st = C8 ? x : ((x >> 12) & 0x0003u);
                                            const uint32_t pr = __builtin_amdgcn_perm(st, tc, selR[sl & 1]);
                                            const uint32_t c = __builtin_amdgcn_inverse_ballot_w64(m) ? pr : 0u;
                                            if (ns == 3 || lane < ns * R) {
                                                MGX_CHECK_LDS_PTR(5, d0 + sl * (V2 * 3), 3);
                                                *reinterpret_cast<uint16_t *>(d16[sl & 1] + sl * (V2 * 3)) = (uint16_t)c;
                                                d8[sl & 1][sl * (V2 * 3)] = (uint8_t)(c >> 16);
                                            }
                                        }
                                    }
                                }
                                continue;
                            }
                        }
                        // whole groups of kG slots, like P2 (padding slots write junk into staging space that P5
                        // never copies): straight-line code whose readlane -> select -> write chains overlap
#pragma unroll
                        for (int g0 = 0; g0 < kR; g0 += kG4) {
                            if (r0 + g0 < NVc) {
#pragma unroll
                                for (int sl = g0; sl < g0 + kG4; ++sl) {
                                    const int s = r0 + sl;
                                    // (see_through_walls: the masks are all ones -- no branch, it would fence the schedule)
                                    // (a pass of at most 32 cells has no high word)
                                    const uint64_t m = (V2 - 64 * it > 32 ? (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visHi[it], s) << 32 : 0ull)
                                                     | (uint64_t)(uint32_t)__builtin_amdgcn_readlane(visLo[it], s);
                                    MGX_CHECK_LDS_PTR(5, d0 + sl * (V2 * 3), 3);
                                    // packed cell(s) -> (type, color) bytes and the state byte (cell_unpack's fields); the pair's
                                    // two ANDs and the shift are common to both of its slots (the compiler keeps them)
                                    const uint32_t x = HALF ? cell[s >> 1][it] : cell[s][it];
                                    const uint32_t tc = C8 ? x : (x & 0x070f070fu), st = C8 ? x : ((x >> 12) & 0x00030003u);
                                    const uint32_t pr = __builtin_amdgcn_perm(st, tc, sel[HALF ? (s & 1) : (sl & 1)]);
                                    const uint32_t c = __builtin_amdgcn_inverse_ballot_w64(m) ? pr : 0u;       // UNSEEN = (0, 0, 0)
                                    *reinterpret_cast<uint16_t *>(d16[sl & 1] + sl * (V2 * 3)) = (uint16_t)c;
                                    d8[sl & 1][sl * (V2 * 3)] = (uint8_t)(c >> 16);                            // ds_write_b8_d16_hi
                                }
                            }
                        }
                    }
                }
                wave_sync();
                // lane r0+sl: its agent's own cell shows the carried object (obs.py:207; always visible, obs.py:252)
                if (lane >= r0 && lane < r0 + kR && lane < NVc)
                    store_obs_cell(outb + (lane - r0) * (V2 * 3) + ((V / 2) * V + (V - 1)) * 3, my_carry);
            }
            wave_sync();
            MGX_MARK("P5");
            if (!MGX_DBG(32)) {
                const int64_t ro0 = o0 + (int64_t)r0 * (V2 * 3);                // this round's obs bytes [ro0, ro1)
                const int rlen = out_skew + (int)min((int64_t)kRoundBytes, o1 - ro0);   // staged bytes, from the aligned start
                uint8_t *gdst = MGX_LATE(obs) + (ro0 - out_skew);
                const __amdgpu_buffer_rsrc_t orsrc = make_rsrc(gdst, rlen);
                constexpr int kPasses = (kRoundBytes + 15 + 1023) / 1024;
#pragma unroll
                for (int k = 0; k < kPasses; ++k) {
                    const int rel = lane16 + 1024 * k;
                    if (rel < rlen) MGX_CHECK_LDS_PTR(6, out_raw + rel, 16);
                    if ((rel + 16 <= rlen) & (rel >= out_skew)) {
                        __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4 *>(out_raw + rel), orsrc, rel, 0,
                                                               PERSIST ? 16 : kObsAux);
                    } else if (rel < rlen) {                                    // ragged head / tail of the wave's bytes
                        const int lo_b = max(rel, out_skew), hi_b = min(rel + 16, rlen);
                        if ((kRoundBytes & 15) != 0 && ((lo_b | hi_b) & 7) == 0) {
                            // (rounds of 8 slots: the round's last / first HALF vector -- every round of a full slice has one)
                            __builtin_amdgcn_raw_buffer_store_b64(*reinterpret_cast<const u32x2 *>(out_raw + lo_b), orsrc, lo_b, 0,
                                                                  PERSIST ? 16 : kObsAux);
                        } else {
#pragma clang loop vectorize(disable) unroll(disable)
                            for (int B = lo_b; B < hi_b; ++B) __builtin_amdgcn_raw_buffer_store_b8(out_raw[B], orsrc, B, 0, PERSIST ? 16 : 0);
                        }
                    }
                }
            }
            wave_sync();
            MGX_MARK("P5end");
        }
    }
    }   // 3-byte staging
    }   // if !OH
    if constexpr (PERSIST) {
        // ------------------------------------------------------------ publish: every output store of this wavefront has left it
        // (write-through) -> its flag says so.  One lane, one relaxed agent-scope store (guide: publish_flag, R1).
#if MGX_SPANS
        const uint64_t t_issued = __builtin_amdgcn_s_memrealtime();      // (every instruction of the step issued; stores in flight)
#endif
        if (NS == 1 || sl_s == ns_act - 1) {                              // (slices: the flag follows the LAST slice's outputs)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(a.done + wid, (uint32_t)t + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        steps_done = t + 1;
        }
#if MGX_SPANS
        // (end stamp: bits [47:0] = the flag store issued, bits [63:48] = ticks the drain before it took)
        const int64_t span_rec = a.span_base + (int64_t)t * gridDim.x * (blockDim.x >> 6) + wid;
        const uint64_t t_flag = __builtin_amdgcn_s_memrealtime();
        if (lane == 0 && span_rec < kSpanCap) g_span[2 * span_rec + 1] = (t_flag & 0xffffffffffffull) | ((t_flag - t_issued) << 48);
#endif
    }
    }   // for t

    if constexpr (GEN && MODE == 1) {
        // -------------------------------------------------------------- the envs whose episode ended with THIS step
        // (base.py:534-539 on the post-step state, which is still in LDS) start their next one here: Agent.reset + _gen_grid
        // by the env's lane, straight into the HBM state (every store of the step itself precedes it in program order)
        // (tested after P1d: done_now / done_mask)
        const uint64_t gmask_all = done_mask;
        uint64_t gmask = gmask_all;                                              // envs generated here, in the tail
        if (gmask_all != 0) MGX_RARE_PATH_PRIO();
        if (gmask_all == 0 && (cand_K > 0 || !stage_tag)) {
            // nothing ended (and no snapshot protocol to serve): the wavefront is done
        } else if (stage_tag && cand_K > 0) {
            // ---------------------------------------------------------- candidates: every finished env whose candidate was there
            // adopts it (a copy; the first one's content came under P2..P5) and advances np_random by the draw that chose it
            const uint64_t amask = cand_mask;
            gmask &= ~amask;
            MGX_SPAN_GFLAG(1, amask != 0);
            if (amask != 0) {
                // the adoption overwrites cells / rows / counters that OTHER lanes of this wavefront stored earlier in the launch (the
                // step's dirty-cell write-back, the agent rows, the step count): those stores must have left the wavefront before
                // these are issued -- the same fence + wait as in front of the tail generation below (rare path; ADVICE r5)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_s_waitcnt(0x0F70);                              // vmcnt(0)
                wave_sync();
                const mgx_gen::NpGen &npr = cand_npr;
                const int r = cand_r;
                for (uint64_t m = amask; m != 0; m &= m - 1) {
                    const int e = __builtin_ctzll(m);                            // wave-uniform
                    const int64_t b = e0 + e, s = b * cand_K + __builtin_amdgcn_readlane(r, e);
                    const uint32_t *sg = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(MGX_LATE_STAGE(grid)) + s * HWB);
                    uint32_t *gg = reinterpret_cast<uint32_t *>(MGX_LATE(grid) + b * HWB);
                    const bool pre = e == pre_e;
                    const uint64_t nrow = pre ? pre_row : (lane < A ? (reinterpret_cast<const uint64_t *>(MGX_LATE_STAGE(agents)) + s * A)[lane] : 0ull);
                    const uint64_t nword = pre ? pre_word : (lane < 5 ? (MGX_LATE_STAGE(words) + s * 6)[lane] : 0ull);
                    uint4 naux = pre_aux;
                    if (HOOKS && !pre) naux = reinterpret_cast<const uint4 *>(MGX_LATE_STAGE(aux))[s];
                    if ((HWB & 3) == 0) {
                        const int nd = HWB / 4;
                        uint32_t v[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = pre ? pre_grid[k] : ((lane + 64 * k < nd) ? sg[lane + 64 * k] : 0u);
#pragma unroll
                        for (int k = 0; k < 4; ++k) if (lane + 64 * k < nd) gg[lane + 64 * k] = v[k];
#pragma unroll 4
                        for (int i = lane + 256; i < nd; i += 64) gg[i] = sg[i];
                    } else {
                        const uint16_t *s16 = reinterpret_cast<const uint16_t *>(sg);
                        uint16_t *g16 = reinterpret_cast<uint16_t *>(gg);
                        for (int i = lane; i < HWB / 2; i += 64) g16[i] = s16[i];
                    }
                    if (lane < A) reinterpret_cast<uint64_t *>(MGX_LATE(agents))[b * A + lane] = nrow;
                    if (lane < 5) MGX_LATE_GEN(gen_state)[b * 6 + lane] = nword;
                    if (lane == e) {
                        if (cand_K > 1) {                                        // np_random after the draw (the increment never changes)
                            MGX_LATE_GEN(gen_state)[b * 6 + 5] = npr.buf;
                            MGX_LATE(rng)[b * 4] = npr.s[0]; MGX_LATE(rng)[b * 4 + 1] = npr.s[1];
                        }
                        if (HOOKS) reinterpret_cast<uint4 *>(MGX_LATE(aux))[b] = naux;
                        MGX_LATE(step_count)[b] = 0;                             // base.py:292
                        MGX_LATE(episode)[b] = (int32_t)in_ep + 1;
                    }
                }
            }
        } else if (stage_tag) {
            // ---------------------------------------------------------- staged generation (include/mgx.h: MgxGenStage)
            const int32_t stage_lead = MGX_LATE_STAGE(lead);                     // (>= 2: the host normalised it)
            // (1) snapshot: an env `lead` steps away from truncation asks for its next episode (the lane of its last agent holds
            // the PCG64 state after this step's draws); the generator wavefronts of the NEXT launch serve it
            const bool in_ = lane < NVc;
            const bool snap = in_ && agent_of_lane == A - 1 && !((gmask_all >> env_of_lane) & 1ull)
                            && scnt[env_of_lane] + 1 == cf.max_steps - stage_lead;
            MGX_SPAN_GFLAG(4, __builtin_amdgcn_ballot_w64(snap) != 0);           // (spans build: 4 = left a snapshot for the generator)
            if (__builtin_amdgcn_ballot_w64(snap) != 0) {
                const uint32_t ep_of_env = (uint32_t)__builtin_amdgcn_ds_bpermute(env_of_lane * 4, (int)in_ep);
                if (snap) {
                    const int64_t b = e0 + env_of_lane;
                    uint64_t *words = MGX_LATE_STAGE(words) + b * 12;
                    words[10] = post_lo; words[11] = post_hi;
                    stage_tag[b * 4 + 1] = (int32_t)ep_of_env;
                    stage_tag[b * 4 + 2] = scnt[env_of_lane] + 1;
                    // (external == 2: the generator launches are serialised with the steps on their stream -- no reader runs beside
                    // this launch, the kernel boundary publishes the snapshot; otherwise the request word goes out last, released:
                    // an agent-scope release writes the XCD's L2 back, ~1.5 us for this wavefront and felt by its neighbours)
                    if (MGX_LATE_STAGE(external) == 2) stage_tag[b * 4 + 3] = MGX_LATE_STAGE(phase) + 1;
                    else __hip_atomic_store(stage_tag + b * 4 + 3, MGX_LATE_STAGE(phase) + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            // (2) adoption: a finished env whose slot holds its episode's successor takes it (a copy: every load of the slot is
            // requested before anything is stored, and waiting for them also waits for the step's own stores to these addresses)
            // (only at the truncation step itself: the slot was generated for np_random as it will be THEN)
            // ... and only a slot made from THIS episode's snapshot at step max_steps - 2: np_random / the step count may have been
            // replaced since (load_state, seed), or the env stepped on past its truncation without auto-reset)
            const bool adopt = done_now && in_tag == (int32_t)in_ep && scnt[lane < Gc ? lane : 0] + 1 == cf.max_steps
                            && in_tag_sc == cf.max_steps - stage_lead;
            const uint64_t amask = __builtin_amdgcn_ballot_w64(adopt);
            gmask &= ~amask;
            MGX_SPAN_GFLAG(1, amask != 0);                                       // (spans build: 1 = adopted a staged episode)
            for (uint64_t m = amask; m != 0; m &= m - 1) {
                const int e = __builtin_ctzll(m);                                // wave-uniform
                const int64_t b = e0 + e;
                const uint32_t *sg = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(MGX_LATE_STAGE(grid)) + b * HWB);
                uint32_t *gg = reinterpret_cast<uint32_t *>(MGX_LATE(grid) + b * HWB);
                const uint64_t *sa = reinterpret_cast<const uint64_t *>(MGX_LATE_STAGE(agents)) + b * A;
                const uint64_t *sw = MGX_LATE_STAGE(words) + b * 12;
                const bool pre = e == pre_e;                                     // (wave-uniform: its content came with P0)
                const uint64_t nrow = pre ? pre_row : (lane < A ? sa[lane] : 0ull);
                const uint64_t nword = pre ? pre_word : (lane < 10 ? sw[lane] : 0ull);
                uint4 naux = pre_aux;
                if (HOOKS && !pre) naux = reinterpret_cast<const uint4 *>(MGX_LATE_STAGE(aux))[b];
                if ((HWB & 3) == 0) {
                    const int nd = HWB / 4;
                    uint32_t v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = pre ? pre_grid[k] : ((lane + 64 * k < nd) ? sg[lane + 64 * k] : 0u);
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (lane + 64 * k < nd) gg[lane + 64 * k] = v[k];
#pragma unroll 4
                    for (int i = lane + 256; i < nd; i += 64) gg[i] = sg[i];
                } else {
                    const uint16_t *s16 = reinterpret_cast<const uint16_t *>(sg);
                    uint16_t *g16 = reinterpret_cast<uint16_t *>(gg);
                    for (int i = lane; i < HWB / 2; i += 64) g16[i] = s16[i];
                }
                if (lane < A) reinterpret_cast<uint64_t *>(MGX_LATE(agents))[b * A + lane] = nrow;
                if (lane < 6) MGX_LATE_GEN(gen_state)[b * 6 + lane] = nword;
                else if (lane < 10) MGX_LATE(rng)[b * 4 + (lane - 6)] = nword;
                if (lane == 0) {
                    if (HOOKS) reinterpret_cast<uint4 *>(MGX_LATE(aux))[b] = naux;
                    MGX_LATE(step_count)[b] = 0;                                 // base.py:292
                    MGX_LATE(episode)[b] = (int32_t)__builtin_amdgcn_readlane(in_ep, e) + 1;
                }
            }
        }
        MGX_SPAN_GFLAG(2, gmask != 0);                                           // (spans build: 2 = generated in the tail)
        if (gmask != 0) {                                   // rare
            MgxLayoutGen gen;
            gen.kind = MGX_LATE_GEN(kind); gen.room_size = MGX_LATE_GEN(room_size);
            gen.start_x = MGX_LATE_GEN(start_x); gen.start_y = MGX_LATE_GEN(start_y); gen.start_dir = MGX_LATE_GEN(start_dir);
            gen.max_hallway_keys = MGX_LATE_GEN(max_hallway_keys); gen.max_keys_per_room = MGX_LATE_GEN(max_keys_per_room);
            gen.blank = MGX_LATE_GEN(blank); gen.gen_state = MGX_LATE_GEN(gen_state);
            done_now = done_now && ((gmask >> lane) & 1ull);                     // (the adopted envs are done with)
            // the env's two generators: the layout stream's six words are requested BEFORE the blank copy and the wait below (one
            // round trip under the other); env.np_random as this step left it is still in registers -- the lane of the env's
            // last agent made it in P0 (post_lo / post_hi; the increment words never change) -- and comes over by ds_bpermute
            mgx_gen::NpGen lay, npr;
            const int64_t gb = e0 + (lane < Gc ? lane : 0);
            uint64_t *const gs = gen.gen_state + gb * 6, *const rg = MGX_LATE(rng) + gb * 4;
            if (done_now) {
                for (int k = 0; k < 4; ++k) lay.s[k] = gs[k];
                lay.buf = gs[4]; npr.buf = gs[5];
            }
            if (A > 1 && !ROLL) {
                const int src_last = ((lane < Gc ? lane : 0) * A + (A - 1)) * 4, src_first = (lane < Gc ? lane : 0) * A * 4;
                auto take64 = [&](const uint64_t v, const int src) -> uint64_t {
                    return ((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(v >> 32)) << 32)
                         | (uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)v);
                };
                npr.s[0] = take64(post_lo, src_last); npr.s[1] = take64(post_hi, src_last);
                npr.s[2] = take64(my_rng[2], src_first); npr.s[3] = take64(my_rng[3], src_first);
            } else if (done_now) {
                // (this launch advanced the env's PCG64 words in P0: read them past the L1)
                for (int k = 0; k < 4; ++k) npr.s[k] = __hip_atomic_load(rg + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            MGX_MARK("G0");
            mgx_gen::copy_blank(gen, MGX_LATE(grid), e0, HWB, gmask, lane);
            // the owning lane now overwrites cells / rows / counters that other lanes of this wavefront stored earlier in the
            // launch (the step's write-back, copy_blank): those stores must have left the wave before its own are issued
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_s_waitcnt(0x0F70);                                  // vmcnt(0)
            wave_sync();
            MGX_MARK("G1");
            if (done_now) {
                const int64_t b = e0 + lane;
                const uint4 naux = mgx_gen::generate_episode(gen, W, H, A, lay, npr, L + cv.rec() + lane * (2 * A),
                                                             MGX_LATE(grid) + b * HWB,
                                                             reinterpret_cast<uint64_t *>(MGX_LATE(agents)) + b * A);
                if (HOOKS) reinterpret_cast<uint4 *>(MGX_LATE(aux))[b] = naux;
                for (int k = 0; k < 4; ++k) { gs[k] = lay.s[k]; rg[k] = npr.s[k]; }
                gs[4] = lay.buf; gs[5] = npr.buf;
                MGX_LATE(step_count)[b] = 0;                                     // base.py:292
                MGX_LATE(episode)[b] += 1;
            }
            MGX_MARK("G2");
        }
    }

#if MGX_TIMESTAMPS
    __builtin_amdgcn_s_waitcnt(0);                       // (the stamps' "end" = the wave's last store retired)
    MGX_MARK("end");
#endif
#if MGX_SPANS
    // (MGX_SPANS alone: "end" = the wave has issued its last instruction; its stores may still be in flight)
    if (!PERSIST && lane == 0 && a.span_base + wid < kSpanCap)
        g_span[2 * (a.span_base + wid) + 1] = (__builtin_amdgcn_s_memrealtime() & 0x0fffffffffffffffull) | (span_flags << 60);
#endif
#undef MGX_SPAN_FLAG
#undef MGX_SPAN_GFLAG
    if (ROLL) {
        // ------------------------------------------------------------------ state write-back, once per launch
        for (int sw = 0; sw < ns_act; ++sw) {
        MGX_SLICE_VARS(sw)
        if constexpr (PITCH != 0) {                                             // the ring-sharing tile: cell by cell
            uint16_t *dst = reinterpret_cast<uint16_t *>(a.grid + e0 * (int64_t)HWB);
            const int HW = H * W;
            for (int c = lane; c < Gc * HW; c += 64) {
                const int e = c / HW, r = c - e * HW, y = r / W, x = r - y * W;
                dst[c] = reinterpret_cast<const uint16_t *>(tile_raw)[e * PITCH * (H - 1) + y * PITCH + x];
            }
        } else
        for (int rel = 16 * lane; rel < len; rel += 16 * 64) {                  // the tile, as it was loaded
            const int64_t D = ga + rel;
            if (D >= g0 && D + 16 <= g1) {
                *reinterpret_cast<uint4 *>(a.grid + D) = *reinterpret_cast<const uint4 *>(tile_raw + rel);
            } else {
                const int64_t lo_b = max(D, g0), hi_b = min(D + 16, g1);
                for (int64_t B = lo_b; B < hi_b; ++B) a.grid[B] = tile_raw[(int)(B - ga)];
            }
        }
        if (lane < NVc) reinterpret_cast<uint64_t *>(a.agents)[v0 + lane] = rows[lane];
        if (A > 1) {
            if (lane < Gc * 4 && (lane & 3) < 2) a.rng[e0 * 4 + lane] = rngs[lane];
            if (lane + 64 < Gc * 4 && (lane & 3) < 2) a.rng[e0 * 4 + lane + 64] = rngs[lane + 64];
        }
        if (lane < Gc) {
            a.step_count[e0 + lane] = scnt[lane];
            if (HOOKS && (AR || env_kind >= MGX_KIND_REDBLUEDOORS)) reinterpret_cast<uint4 *>(a.aux)[e0 + lane] = auxl[lane];
        }
        }   // for sw
        if constexpr (PERSIST) {            // how far the launch got: [2] += wavefronts that have left, [3] = min over them of their steps
            if (lane == 0) { atomicAdd(a.pctrl + 2, 1u); atomicMin(a.pctrl + 3, (uint32_t)steps_done); }
        }
    }
#undef MGX_SLICE_VARS
#undef lane
#undef MGX_LATE_GEN
#undef MGX_LATE_STAGE
#undef MGX_PUB_STORE_U8
