// The body of score_kernel, score_rowfrag_kernel and score_colfrag_kernel (csrc/score.hip), included INSIDE each: one text for all, and the
// kernels compile exactly as if each had it written out (as a function inlined into two wrappers, every instantiation came out
// with other code).  It sees the kernel's argument `ScoreArgs p` and D, MODE_T, HAS_IDS, HAS_HN, WAVES, PREC as compile-time constants.
  // FAST: the two instantiations of the plain train step.  What they leave out is work on values the step's arguments make dead:
  //  * MODE_BWD_S_NR: `+ a_r` (a zero) and `* s_r` (a one) on every element; a_c / s_c are given, so their staging has no selects.
  //  * MODE_FUSED_S_NC: the column bias altogether - no staging load, no LDS write, no LDS read; X * c1 instead of fma(X, c1, 0).
  //  * both: the tile loop is cut in two.  The MAIN loop runs the tiles whose own 32 streamed rows AND those of the tiles it
  //    prefetches are all valid: no row clamps on the loads, no zeroing selects in store_tile, no mask_S, no tile-index clamp.  The
  //    TAIL loop (the last 2-4 tiles of the split, the possibly ragged one among them) is the general step with all of these.
  //    Which lanes need masking for what is stored: a lane whose stationary row r >= n_r feeds only column r of the gradient
  //    block (the coefficient is the B operand: MFMA output column j depends on B column j alone), and that column is dropped at
  //    the slab store - no mask needed.  Only an invalid STREAMED row (a register of X, a row of the LDS tile) is summed into
  //    valid outputs, and invalid streamed rows exist in a split's last tile only.
  //  * both: nothing wave-uniform or constant is computed on the vector ALU per tile - the per-tile bases are SGPR pairs
  //    (uniform_base) beside one loop-invariant 32-bit VGPR offset, the positive-tile test is two scalar compares of the tile index.
  //  * MODE_BWD_S_NR at D <= 128: a_c / s_c of the split's streamed rows are staged ONCE, in the prologue, into an LDS array
  //    (ROW_LDS); MODE_BWD_S_NR_T stages them per tile, for splits longer than the array.
  constexpr int MODE = base_mode(MODE_T);
  constexpr bool FAST = MODE_T != MODE;
  static_assert(!FAST || (PREC == 0 && !HAS_IDS && !HAS_HN), "the fast forms: exact f32, no ids, no hard negatives");
  // WG: MODE_FUSED_S_NC's arithmetic, one 32-row fragment per workgroup: wave w = column split w (nsplit == WAVES: launch_score
  // checks).  What differs is where a wave's tiles live (a private LDS buffer, no workgroup barrier) and where the splits meet (LDS).
  constexpr bool WG = MODE_T == MODE_FUSED_S_WG;
  static_assert(!WG || (D == 128 && WAVES == 8), "splits inside the workgroup: dim 128, 8 waves");
  // CW: MODE_BWD_S_NR_T's arithmetic, one 32-row fragment of the stationary side (the candidates) per workgroup: wave w = split w of
  // the streamed queries (nsplit == WAVES, n_c == WAVES * c_per_split - whole tiles, the same number for every wave: launch_score
  // checks).  As in WG, a wave's tiles live in a private LDS buffer (no workgroup barrier) and the splits meet in LDS.
  constexpr bool CW = MODE_T == MODE_BWD_S_WG;
  static_assert(!CW || (D == 128 && WAVES == 8), "splits inside the workgroup: dim 128, 8 waves");
  constexpr bool INWG = WG || CW;                        // one fragment per workgroup, wave = split, private tiles
  constexpr BoolC<false> GEN{};                            // the general form of a step: every clamp and select
  constexpr BoolC<true> FULL_TILE{};
  constexpr bool NO_AC = FAST && MODE == MODE_FUSED_S;      // no column bias: nothing staged for it
  constexpr bool NO_ROW = FAST && MODE == MODE_BWD_S;       // no row bias / scale; column bias and scale are non-null
  // ROW_LDS: a_c / s_c of the split's streamed rows sit in one LDS array behind the tile ring, written once in the prologue: the
  // tile loops load and stage no side values at all (a workgroup uses the same c_per_split values for the whole launch)
  constexpr bool ROW_LDS = row_terms_in_lds<D, MODE_T>();
  constexpr bool IS_FUSED = MODE == MODE_FUSED || MODE == MODE_FUSED_S;     // online softmax + dq
  constexpr bool IS_BWD = MODE == MODE_BWD || MODE == MODE_BWD_S;            // gradient pass with given row statistics
  constexpr bool FROM_S = MODE == MODE_BWD_S, TO_S = MODE == MODE_FUSED_S;
  using G_ = Geo<D, PREC>;
  constexpr int LS = G_::LS, NG = G_::NG, NB = G_::NB, TILE_F = G_::TILE_F, BUF_F = G_::BUF_F;
  constexpr int HALF_B = G_::HALF_B, PIECE_B = G_::PIECE_B;
  constexpr bool SPLIT = split_d<D, MODE, PREC>();
  constexpr int KS = SPLIT ? G_::KS / 2 : G_::KS;     // GEMM1 k-steps of THIS wave
  constexpr int NBW = SPLIT ? NB / 2 : NB;            // GEMM2 d-blocks of THIS wave
  static_assert(PREC == 0 || D % 128 == 0, "bf16x3: dim 128 / 256 only (whole [32][128] bf16 images)");
  constexpr int ROW4 = D / 4;                       // float4 per K row
  constexpr int THREADS = WAVES * 64;
  constexpr int NV = (32 * ROW4 + THREADS - 1) / THREADS;   // staged float4 per thread
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // (FAST: the wave index as a scalar, so that the fragment's first row, the positive-tile test and the block addresses of the
  // stored dot products are SALU work; the general kernels keep the vector copy they were tuned with)
  const int wave = FAST ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  const int h = lane >> 5;
  const int ln = lane & 31;

  // Everything that steers a loop with a workgroup barrier in it is made PROVABLY wave-uniform (readfirstlane): the split,
  // the row block and, below, the tile count.  They depend on blockIdx and kernel arguments only, but hipcc divides on the
  // vector ALU; whether the quotient comes back to an SGPR is its choice, and a trip count left in VGPRs turns the tile
  // loop's exit test into a vector compare with the barrier inside a loop the compiler treats as divergent.
  // tests/isa_audit/audit_barriers.py checks the built ISA: in all instantiations every barrier loop closes on scalar branches.
  const int split = __builtin_amdgcn_readfirstlane(INWG ? wave : (int)(blockIdx.x % (unsigned)p.nsplit));
  const int64_t rblk = __builtin_amdgcn_readfirstlane(INWG ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)p.nsplit));
  const int hw = SPLIT ? (wave & 1) : 0;             // SPLIT: the half of the embedding dimension this wave owns
  const int64_t r0w = INWG ? rblk * 32               // first row of this wave (WG / CW: of all 8)
                         : rblk * rows_per_wg<D, MODE, PREC, WAVES>() + (SPLIT ? wave >> 1 : wave) * 32;
  const int64_t r = r0w + ln;                       // this lane's row (both halves)
  const bool r_ok = r < p.n_r;
  const int64_t c_begin = (int64_t)split * p.c_per_split;
  int64_t c_end = c_begin + p.c_per_split;
  if (c_end > p.n_c) c_end = p.n_c;
  const int ntiles = __builtin_amdgcn_readfirstlane(c_end > c_begin ? (int)((c_end - c_begin + 31) >> 5) : 0);
  const int nfull = __builtin_amdgcn_readfirstlane(c_end > c_begin ? (int)((c_end - c_begin) >> 5) : 0);   // tiles of 32 valid rows (FAST)

  // ---- stationary fragment (B operand of GEMM1), in registers for the whole launch ----
  //   f32:     rf[g][s]     = R[r][8g + 4h + s]
  //   bf16x3:  rp[q][ks][j] = piece q of R[r][16 ks + 8h + j]
  // (bf16x3 with 8-wave workgroups: the lo piece — one product per k-step — lives in LDS, [ks][lane] x 16 B per wave,
  // written once: 32 VGPRs less, which is what keeps the gradient kernels free of scratch spills)
  constexpr bool RLO_LDS = PREC == 1 && WAVES == 8;
  // exact-f32 gradient passes: TPB tiles between workgroup barriers (ring of 2*TPB LDS buffers, the prefetch runs TPB tiles
  // ahead); everything else: one tile per barrier, two buffers
  constexpr int TPB = tiles_per_barrier<D, MODE, PREC>();
  // Two LDS assumptions of the wave-pair (SPLIT) path, pinned: its exchange buffer `xch` sits where the 8-wave kernels keep the
  // lo fragments (`rlo`) - never both in one kernel; and exchange() has ONE barrier between a pair's write and its partner's
  // read, so the next tile's write is only safe behind the per-tile barrier that TPB == 1 gives.
  static_assert(!(SPLIT && RLO_LDS), "wave-pair exchange buffer and the LDS lo fragments share one LDS region");
  static_assert(!SPLIT || TPB == 1, "the wave-pair exchange relies on one workgroup barrier per tile");
  constexpr int NBUF = 2 * TPB;
  constexpr int RFL = rf_lds_groups<D, MODE, HAS_IDS, HAS_HN, PREC>();      // k-groups of the stationary fragment kept in LDS
  constexpr int RFR = PREC == 0 ? NG - RFL : 1;                             // ... and in registers
  f32x4 rf[RFR];
  f32x4* rfl = reinterpret_cast<f32x4*>(smem + NBUF * BUF_F) + (wave * (RFL > 0 ? RFL : 1)) * 64 + lane;   // [group][lane], this wave's
  bf16x8 rp[PREC == 0 ? 1 : (RLO_LDS ? 2 : 3)][PREC == 0 ? 1 : KS];
  bf16x8* rlo = reinterpret_cast<bf16x8*>(smem + NBUF * BUF_F) + (wave * KS) * 64 + lane;
  if constexpr (FROM_S) {
    // pass 2 of the training entry: the dot products come back from HBM, no stationary fragment, no GEMM1
  } else if constexpr (PREC == 0) {
    const f32x4* R4 = reinterpret_cast<const f32x4*>(p.R + (r_ok ? r : 0) * D) + h;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const f32x4 v = r_ok ? R4[2 * g] : f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (RFL > 0) {
        if (g >= RFR) rfl[(g - RFR) * 64] = v; else rf[g < RFR ? g : 0] = v;   // (read back by this lane only: no barrier needed)
      } else {
        rf[g] = v;
      }
    }
  } else {
    const f32x4* R4 = reinterpret_cast<const f32x4*>(p.R + (r_ok ? r : 0) * D) + 2 * h + 32 * hw;
    const float live = r_ok ? 1.f : 0.f;            // rows past n_r read row 0 and are zeroed (all loads unconditional)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const f32x4 x0 = R4[4 * ks] * live;
      const f32x4 x1 = R4[4 * ks + 1] * live;
      bf16x8 lo8;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const Bf3 u = split3(x0[j]), v = split3(x1[j]);
        rp[0][ks][j] = u.hi; rp[1][ks][j] = u.mid; lo8[j] = u.lo;
        rp[0][ks][4 + j] = v.hi; rp[1][ks][4 + j] = v.mid; lo8[4 + j] = v.lo;
      }
      if constexpr (RLO_LDS) rlo[ks * 64] = lo8;        // read back by this lane only: no barrier needed
      else rp[2][ks] = lo8;
    }
  }
  const float ar = (!NO_ROW && (IS_BWD || MODE == MODE_RANK) && p.a_r != nullptr && r_ok) ? p.a_r[r] : 0.f;
  const float sr = (!NO_ROW && IS_BWD && p.s_r != nullptr && r_ok) ? p.s_r[r] : 1.f;
  int64_t idr = 0;
  if constexpr (HAS_IDS) idr = r_ok ? p.id_r[r] : (int64_t)-1;
  const int64_t cpos = p.pos_idx != nullptr ? (r_ok ? p.pos_idx[r] : (int64_t)-1) : r + p.diag;   // positive column
  // FAST (no explicit positives: launch_score checks): the positive-tile test as two scalar 32-bit compares on the tile index.
  // d = r0w + diag - c_begin is where the fragment's first positive sits in the split; tile t holds a positive of the fragment iff
  // -32 < d - 32 t < 32, i.e. floor(d / 32) <= t <= floor((d + 31) / 32) (clamped to the tile indices an int holds; an empty range
  // where none qualifies).  Inside such a tile the lane's positive row is ln + (d - 32 t), a small number, taken modulo 2^32.
  const int64_t dfrag = r0w + p.diag - c_begin;
  const int64_t dt_lo64 = dfrag >> 5, dt_hi64 = (dfrag + 31) >> 5;
  const bool dt_none = dt_hi64 < 0 || dt_lo64 > 0x7fffffff;
  const int dt_lo = FAST ? __builtin_amdgcn_readfirstlane(dt_none ? 1 : (dt_lo64 < 0 ? 0 : (int)dt_lo64)) : 0;
  const int dt_hi = FAST ? __builtin_amdgcn_readfirstlane(dt_none ? 0 : (dt_hi64 > 0x7fffffff ? 0x7fffffff : (int)dt_hi64)) : 0;
  const unsigned dfrag_lo = FAST ? (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)dfrag) : 0u;
  const int lnh = ln - 4 * h;
  const int xor32_addr = (lane ^ 32) << 2;            // ds_bpermute address of the lane that holds the row's other half

  // ---- staging (global -> regs -> LDS, TPB tiles ahead).  Thread `tid` moves float4 number
  // tid + THREADS*j of the tile (row = f / ROW4, col4 = f % ROW4).
  // Every load of the tile loop is UNCONDITIONAL, from a clamped (valid) address, and what a lane must not see is replaced by a
  // select where the registers are consumed (store_tile, mask_S).  Written as `x = ok ? p[i] : 0`, each load sat in an exec-mask
  // region of its own, and with one load of the loop under a condition - a lane mask or a uniform `if` alike - the compiler cannot
  // count the loads YOUNGER than the one it waits for: every wait of the loop was `s_waitcnt vmcnt(0)`, which also drains the
  // prefetches just issued (tests/isa_audit/audit_score_loads.py).  So the callers clamp the tile index
  // (past the end a wave reads its last tile again, an L1 / L2 hit nobody consumes) and skip only the store_tile / the use.
  f32x4 st[NV];
  float st_a = 0.f, st_s = 0.f, st_h = -3.0e38f;
  constexpr bool hn = HAS_HN;                                        // hard-negative mining compiled in
  const float hr = (HAS_HN && p.h_r != nullptr && r_ok) ? p.h_r[r] : -3.0e38f;
  int64_t st_id = -2;
  constexpr int RPJ = THREADS / ROW4 > 0 ? THREADS / ROW4 : 1;   // tile rows between a thread's consecutive float4s
  const int st_row = tid / ROW4, st_col4 = tid % ROW4;
  const f32x4* kp = reinterpret_cast<const f32x4*>(p.K) + c_begin * ROW4;   // tile 0
  // the nullable per-column vectors: a null one is read from K instead (n_c * D floats, so [c_begin + 32 t + row] exists) and
  // its value dropped in store_tile
  const bool has_ac = p.a_c != nullptr, has_sc = p.s_c != nullptr, has_hc = HAS_HN && p.h_c != nullptr;
  const float* acp = (has_ac ? p.a_c : p.K) + c_begin;
  const float* scp = (has_sc ? p.s_c : p.K) + c_begin;
  const float* hcp = (has_hc ? p.h_c : p.K) + c_begin;
  const int64_t* idp = nullptr;
  if constexpr (HAS_IDS) idp = p.id_c + c_begin;
  const int ncols = (int)(c_end - c_begin);         // columns of this split (<= c_per_split)

  constexpr bool ST_FULL = NV * THREADS == 32 * ROW4;              // every thread stages NV float4 of every tile
  // FAST: the byte offset of the thread's float4 within a full tile, kept in a register of its own (not recomputed from tid at
  // every load)
  unsigned st_offb = 16u * (unsigned)((ST_FULL ? st_row : (st_row < 31 ? st_row : 31)) * ROW4 + st_col4);
  // t: a tile that exists (0 <= t < ntiles).  Rows past the tile's last valid row read that row.
  // full (FAST kernels' main loop): tile t has 32 valid rows - `last` is the constant 31, the clamps are loop-invariant.
  auto load_tile = [&](int t, auto full) {
    constexpr bool FULL = decltype(full)::value;
    const f32x4* src = kp + (int64_t)t * (32 * ROW4);
    if constexpr (FULL) {
      // a wave-uniform base per tile and per j (an SGPR pair, see uniform_base) + one loop-invariant unsigned 32-bit offset per
      // thread: no VALU per tile
      static_assert(ST_FULL || NV == 1, "threads past row 31 exist only where a thread stages one float4");
      // (a base per j as well: j * RPJ rows are 8 KB and more, past what the load's immediate offset holds.  The 32-bit offset is
      // widened HERE, beside the loads: hoisted out of the loop as a 64-bit value it no longer fits the load's offset operand.)
      asm volatile("" : "+v"(st_offb));
#pragma unroll
      for (int j = 0; j < NV; ++j)
        st[j] = *(global_ptr<const f32x4>)((global_ptr<const char>)uniform_base(src + (ST_FULL ? j * RPJ * ROW4 : 0)) + st_offb);
      const unsigned c31 = (unsigned)(tid < 31 ? tid : 31);
      if constexpr (!NO_AC && !ROW_LDS) st_a = uniform_base(acp + 32 * (int64_t)t)[c31];
      if constexpr (IS_BWD && !ROW_LDS) st_s = uniform_base(scp + 32 * (int64_t)t)[c31];
      return;
    }
    const int nvalid = ncols - 32 * t;              // valid rows of tile t (may exceed 32)
    const int last = (nvalid < 32 ? nvalid : 32) - 1;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int row = st_row + j * RPJ;
      st[j] = src[(row < last ? row : last) * ROW4 + st_col4];
    }
    const int c = 32 * t + (tid < last ? tid : last);
    if constexpr (!NO_AC && !ROW_LDS) st_a = acp[c];
    if constexpr (HAS_HN) st_h = hcp[c];
    if constexpr (IS_BWD && !ROW_LDS) st_s = scp[c];  // (the only passes whose epilogue reads s_c)
    if constexpr (HAS_IDS) st_id = idp[c];
  };
  // t: the tile the staging registers were loaded for.  Past the split's end (t >= ntiles: the registers hold the last tile
  // again) the store is NOT skipped: buffer t % NBUF is free by then, nobody reads what lands in it, and a load that is
  // consumed on every path is what lets the compiler drop the full waits at the top of the loop (a staging register still
  // pending there on some path forced `s_waitcnt vmcnt(0)` in front of the first VALU write that reuses one).
  // The same holds for the lanes: the side values are written by 32 threads only (and at dim 32 with 8 waves half the threads
  // stage nothing), so every thread "uses" its staging registers in an empty asm statement - no instruction, but the wait for
  // the load now stands at the store_tile on every path instead of as a vmcnt(0) wherever the register is written next.
  // full: the staging registers hold a tile of 32 valid rows - nothing to zero (threads past row 31 store nothing, as ever).
  auto store_tile = [&](int t, int buf, auto full) {
    constexpr bool FULL = decltype(full)::value;
    float* T = smem + buf * BUF_F;
    const int nvalid = ncols - 32 * t;
    if constexpr (!FULL) {
#pragma unroll
      for (int j = 0; j < NV; ++j) st[j] = (st_row + j * RPJ < nvalid) ? st[j] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (!ST_FULL) {
#pragma unroll
      for (int j = 0; j < NV; ++j) asm volatile("" : : "v"(st[j]));
    }
    if constexpr (PREC == 0) {
      float* dst = T + st_row * LS + st_col4 * 4;
#pragma unroll
      for (int j = 0; j < NV; ++j)
        if (ST_FULL || st_row + j * RPJ < 32) *reinterpret_cast<f32x4*>(dst + j * RPJ * LS) = st[j];
    } else {
      // three bf16 images of the tile (hi / mid / lo pieces), each float4 -> 4 bf16 = one ds_write_b64 per piece
      char* img = reinterpret_cast<char*>(T);
      const int d0 = 4 * st_col4;
      const int sub = (d0 >> 7) * HALF_B + 8 * ((d0 >> 2) & 1), ch = (d0 & 127) >> 3;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int row = st_row + j * RPJ;
        if (ST_FULL || row < 32) {
          bf16x4 q0, q1, q2;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const Bf3 u = split3(st[j][e]);
            q0[e] = u.hi; q1[e] = u.mid; q2[e] = u.lo;
          }
          char* dst = img + sub + img_off(row, ch);
          *reinterpret_cast<bf16x4*>(dst) = q0;
          *reinterpret_cast<bf16x4*>(dst + PIECE_B) = q1;
          *reinterpret_cast<bf16x4*>(dst + 2 * PIECE_B) = q2;
        }
      }
    }
    if constexpr (NO_AC || ROW_LDS) {
      return;                                          // no side values at all: the epilogue derives the bias (0 / -big) from t (NO_AC)
                                                       // or reads the row terms from the workgroup's LDS array (ROW_LDS)
    } else if constexpr (NO_ROW) {
      asm volatile("" : : "v"(st_a));
      asm volatile("" : : "v"(st_s));
      if (tid < 32) {                                  // a_c and s_c are given (launch_score checks)
        const bool ok = FULL || tid < nvalid;
        T[TILE_F + tid] = ok ? st_a : kNegBig;
        T[TILE_F + 32 + tid] = ok ? st_s : 0.f;
      }
      return;
    }
    asm volatile("" : : "v"(st_a));
    if constexpr (IS_BWD) asm volatile("" : : "v"(st_s));
    if constexpr (HAS_HN) asm volatile("" : : "v"(st_h));
    if constexpr (HAS_IDS) asm volatile("" : : "v"(st_id));
    if (tid < 32) {
      const bool ok = tid < nvalid;
      T[TILE_F + tid] = ok ? (has_ac ? st_a : 0.f) : kNegBig;
      T[TILE_F + 32 + tid] = ok ? ((IS_BWD && has_sc) ? st_s : 1.f) : 0.f;
      if constexpr (HAS_HN) T[TILE_F + 128 + tid] = (ok && has_hc) ? st_h : -3.0e38f;
      if constexpr (HAS_IDS) reinterpret_cast<int64_t*>(T + TILE_F + 64)[tid] = ok ? st_id : (int64_t)-2;
    }
  };

  // ---- WG: the wave's PRIVATE tile.  One LDS buffer of 32 x LS floats per wave (eight of them: 135 KB; a second one per wave does
  // not fit the 160 KB), and no register set for a whole tile either: 16 float4 per lane (64 registers) beside the fragment (64),
  // the gradient block (64) and what a tile step needs leave nothing of the 256.  So the split's tiles are streamed as CHUNKS of 8 rows (four float4 per lane: lane =
  // (row & 1, float4 column), j = row pair), two chunks in flight in two register sets.  GEMM2 reads its tile for the last time
  // in row order - the steps reg = 4k .. 4k+3 read rows 8k .. 8k+7 - so behind them chunk k of the NEXT tile is written over those
  // rows and the stream's chunk after next requested into the freed registers: every chunk has half a GEMM2 (a microsecond and
  // more) between request and use, GEMM1 of the next tile starts behind the last quarter's write.  A wave's LDS operations
  // execute in order, the buffer is its own: no barrier.  Loads unconditional from clamped addresses, as everywhere.
  // CW: the same chunk stream with the tile's 64 row terms (a_c | s_c, where the epilogue looks for them) behind each wave's tile;
  // it has no GEMM1, no stationary fragment and only full tiles.
  constexpr int WBUF_F = CW ? TILE_F + 64 : TILE_F;    // floats of a wave's private buffer
  float* TW = smem + (INWG ? wave * WBUF_F : 0);
  f32x4 ck[2][4];
  unsigned ck_offb = 16u * (unsigned)lane;             // byte offset of the lane's float4 within a row pair
  // t: a tile that exists; k: chunk 0 .. 3.  full: tile t has 32 valid rows - a scalar base and immediate offsets, no clamp
  auto load_chunk = [&](f32x4 (&s)[4], int t, int k, auto full) {
    constexpr bool FULL = decltype(full)::value;
    const f32x4* src = kp + (int64_t)t * (32 * ROW4) + k * (8 * ROW4);
    if constexpr (FULL) {
      asm volatile("" : "+v"(ck_offb));
      const global_ptr<const char> base = (global_ptr<const char>)uniform_base(src);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = *(global_ptr<const f32x4>)(base + ck_offb + j * (2 * ROW4 * 16));
      return;
    }
    // a row past the tile's last valid row reads that row: the same scalar base (the tile's), a clamped 32-bit offset per float4
    const int nvalid = ncols - 32 * t;                 // valid rows of tile t (may exceed 32)
    const int last = (nvalid < 32 ? nvalid : 32) - 1;
    const global_ptr<const char> base = (global_ptr<const char>)uniform_base(kp + (int64_t)t * (32 * ROW4));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 8 * k + 2 * j + h;
      s[j] = *(global_ptr<const f32x4>)(base + 16u * (unsigned)((row < last ? row : last) * ROW4 + ln));
    }
  };
  // t: the tile the registers were loaded for; past the split's end (t >= ntiles: they hold the last tile again) every row is zeroed
  // and lands in a buffer nobody reads again (see store_tile)
  auto store_chunk = [&](f32x4 (&s)[4], int t, int k, auto full) {
    constexpr bool FULL = decltype(full)::value;
    const int nvalid = ncols - 32 * t - 8 * k;
    float* dst = TW + (8 * k + h) * LS + 4 * ln;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 v = (FULL || 2 * j + h < nvalid) ? s[j] : f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(dst + 2 * j * LS) = v;
    }
  };

  // ---- the raw dot products through HBM (training entry: pass 1 writes them, pass 2 reads them back) ----
  // Stored as 32 x 32 BLOCKS of 4 KB, block (candidate tile, query tile) at [ctile * ldS + qtile] (ldS = query tiles), inside a
  // block [query][candidate]: the block one wave produces in pass 1 is the block one wave consumes in pass 2, and both
  // move it as one contiguous 4 KB burst (row-major [nq][nc] made every 128-byte line of a tile a separate DRAM page).
  // FUSED_S (R = q, K = c): lane = query row, accumulator register reg = candidate acc_row(reg, h): registers 4g .. 4g+3
  //   are 4 consecutive candidates -> one 16-byte store per g.
  // BWD_S (R = c, K = q): lane = candidate, register = query row: for a fixed register the 32 lanes of a half read 32
  //   consecutive candidates of one query row -> coalesced 4-byte loads.
  // (r02 alternatives, cfg3, pass 1 / pass 2 us against 287 / 174 for row-major: transposed row-major 290 / 170;
  // nontemporal stores 387 / 175 - the pieces of a line are no longer merged in L2; nontemporal loads 287 / 175.)
  // A fragment with a valid row has its blocks (ws_layout allocates whole blocks), so its rows past n_r are stored too - pass 2
  // masks them - and the stores sit under no lane mask; a fragment with no valid row at all has none (wave-uniform).
  const bool frag_ok = __builtin_amdgcn_readfirstlane((int)(r0w < p.n_r)) != 0;
  auto store_S = [&](int t, const f32x16& X) {
    if (!WG && !frag_ok) return;                      // (WG: one fragment per workgroup, the grid holds none without a valid row)
    const int64_t ctile = (c_begin >> 5) + t;
    if constexpr (FAST) {                              // wave-uniform block address + a loop-invariant 32-bit lane offset
      const global_ptr<f32x4> blk_u = uniform_base(reinterpret_cast<f32x4*>(p.S + (ctile * p.ldS + (r0w >> 5)) * 1024));
      const unsigned lo4 = (unsigned)(ln * 8 + h);
#pragma unroll
      for (int g = 0; g < 4; ++g) (blk_u + 2 * g)[lo4] = f32x4{X[4 * g], X[4 * g + 1], X[4 * g + 2], X[4 * g + 3]};
      return;
    }
    float* blk = p.S + (ctile * p.ldS + (r0w >> 5)) * 1024 + ln * 32 + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (!SPLIT || (g >> 1) == hw)       // SPLIT: both waves of the pair hold the same block, each stores half of it
        *reinterpret_cast<f32x4*>(blk + 8 * g) = f32x4{X[4 * g], X[4 * g + 1], X[4 * g + 2], X[4 * g + 3]};
  };
  // SPLIT: the partial dot products of the two k-halves meet in LDS.  a + b == b + a bit for bit, so both waves of a pair go
  // on with the same block (their softmax statistics are duplicates, their gradient columns disjoint).
  float* xch = smem + NBUF * BUF_F;
  auto exchange = [&](f32x16& X) {
    f32x4* mine = reinterpret_cast<f32x4*>(xch + wave * 1024) + lane;
    const f32x4* other = reinterpret_cast<const f32x4*>(xch + (wave ^ 1) * 1024) + lane;
#pragma unroll
    for (int g = 0; g < 4; ++g) mine[64 * g] = f32x4{X[4 * g], X[4 * g + 1], X[4 * g + 2], X[4 * g + 3]};
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 o = other[64 * g];
#pragma unroll
      for (int i = 0; i < 4; ++i) X[4 * g + i] += o[i];
    }
  };
  // t: a tile that exists.  16 unconditional loads from a block that exists: S is allocated in whole 32 x 32 blocks, so every
  // element of the block of a fragment with a valid row may be read; a fragment with none reads row block 0.  What the lanes and
  // rows past the ends read is uninitialised workspace: mask_S replaces it (a select - it may be NaN) where tile t is consumed.
  auto load_S = [&](int t, f32x16& X) {
    const int64_t q0 = c_begin + 32 * (int64_t)t;
    if constexpr (FAST) {                              // wave-uniform block address + a loop-invariant 32-bit lane offset
      const global_ptr<const float> blk_u = uniform_base((const float*)p.S + ((frag_ok ? (r0w >> 5) : 0) * p.ldS + (q0 >> 5)) * 1024);
      const unsigned lo = (unsigned)(4 * h * 32 + ln);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) X[reg] = (blk_u + tt::acc_row(reg, 0) * 32)[lo];
      return;
    }
    const float* blk = p.S + ((frag_ok ? (r0w >> 5) : 0) * p.ldS + (q0 >> 5)) * 1024 + 4 * h * 32 + ln;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) X[reg] = blk[tt::acc_row(reg, 0) * 32];
  };
  auto mask_S = [&](int t, const f32x16& Xin) -> f32x16 {
    const int nq_left = ncols - 32 * t;               // valid query rows of this tile (may exceed 32)
    f32x16 X;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) X[reg] = (r_ok && (tt::acc_row(reg, 0) + 4 * h) < nq_left) ? Xin[reg] : 0.f;
    return X;
  };
  auto clamp_tile = [&](int t) { return t < ntiles ? t : ntiles - 1; };     // (callers are inside `ntiles > 0`)

  // ---- per-lane state ----
  float run_m = kNegBig, run_l = 0.f, pos = 0.f;
  int cnt = 0;
  bool have_pos = false;
  f32x16 G[NBW];
  if constexpr (IS_BWD || IS_FUSED) {
#pragma unroll
    for (int b = 0; b < NBW; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) G[b][i] = 0.f;
  }

  // (r02: starting the second workgroup of every CU 1-4 us late, so that the two waves of a SIMD run half a tile apart, only
  // added the delay: 174.9 -> 175.5 .. 177.7 us for the dc pass.  Ablation of that pass: GEMM2 alone 112 us = the matrix pipe's
  // time; everything else - tile staging 25, dot-product loads 6-19, epilogue 9, loop skeleton 23 - adds to it instead of
  // hiding under it, with or without a phase shift between the waves.)
  // ROW_LDS: the row terms of the split's ntiles * 32 streamed rows, [a_c | s_c] with kRowTermRows floats each, behind the tile ring.
  // Two rows per thread and trip, all four loads unconditional from clamped indices; a row past the split's end gets what
  // store_tile stages for it (-big, 0).  launch_score takes this form only where c_per_split <= kRowTermRows.  The barrier below
  // publishes the array with the first tiles.
  float* rowterm = smem + NBUF * BUF_F;
  if constexpr (ROW_LDS) {
    const int nrt = 32 * ntiles;
    for (int i0 = 0; i0 < nrt; i0 += 2 * THREADS) {
      const int i_a = i0 + tid, i_b = i0 + THREADS + tid;
      const int c_a = i_a < ncols ? i_a : ncols - 1, c_b = i_b < ncols ? i_b : ncols - 1;     // (nrt > 0: ncols >= 1)
      const float a_a = acp[c_a], s_a = scp[c_a], a_b = acp[c_b], s_b = scp[c_b];
      if (i_a < nrt) {
        rowterm[i_a] = i_a < ncols ? a_a : kNegBig;
        rowterm[kRowTermRows + i_a] = i_a < ncols ? s_a : 0.f;
      }
      if (i_b < nrt) {
        rowterm[i_b] = i_b < ncols ? a_b : kNegBig;
        rowterm[kRowTermRows + i_b] = i_b < ncols ? s_b : 0.f;
      }
    }
  }
  if constexpr (!INWG) {
#pragma unroll
    for (int t0 = 0; t0 < TPB; ++t0)
      if (t0 < ntiles) {
        load_tile(t0, GEN);
        store_tile(t0, t0, GEN);
      }
    __syncthreads();
  }
  // ---- GEMM1: X[c][r] = sum_d K[c][d] R[r][d] ----
  auto gemm1 = [&](const float* T) -> f32x16 {
    f32x16 X;
#pragma unroll
    for (int i = 0; i < 16; ++i) X[i] = 0.f;
    if constexpr (PREC == 1) {
      // A operand: lane (row c = ln, half h) reads k = 16 ks + 8h .. +7 of every piece: one ds_read_b128 per piece.
      // Software-pipelined by hand: the three fragments of k-step ks+1 are in flight under the six MFMAs of k-step ks
      // (left to the compiler the MFMAs sat behind each read's LDS latency: 2.3x the pure MFMA time, r02 ablation).
      const char* img = reinterpret_cast<const char*>(T);
      auto frag = [&](int ks, bf16x8& f_hi, bf16x8& f_mid, bf16x8& f_lo, bf16x8& r_lo) {
        const int off = (SPLIT ? hw : (ks >> 3)) * HALF_B + img_off(ln, 2 * (ks & 7) + h);
        f_hi = *reinterpret_cast<const bf16x8*>(img + off);
        f_mid = *reinterpret_cast<const bf16x8*>(img + PIECE_B + off);
        f_lo = *reinterpret_cast<const bf16x8*>(img + 2 * PIECE_B + off);
        if constexpr (RLO_LDS) r_lo = rlo[ks * 64];
      };
      bf16x8 a_hi, a_mid, a_lo, b_lo = {};
      frag(0, a_hi, a_mid, a_lo, b_lo);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        bf16x8 n_hi = a_hi, n_mid = a_mid, n_lo = a_lo, nb_lo = b_lo;
        if (ks + 1 < KS) frag(ks + 1, n_hi, n_mid, n_lo, nb_lo);
        if constexpr (!RLO_LDS) b_lo = rp[2][ks];
        X = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, rp[0][ks], X, 0, 0, 0);     // smallest terms first
        X = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, X, 0, 0, 0);
        X = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_mid, rp[1][ks], X, 0, 0, 0);
        X = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_mid, rp[0][ks], X, 0, 0, 0);
        X = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, rp[1][ks], X, 0, 0, 0);
        X = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, rp[0][ks], X, 0, 0, 0);
        a_hi = n_hi; a_mid = n_mid; a_lo = n_lo; b_lo = nb_lo;
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      const float* arow = T + ln * LS + 4 * h;
      // one ds_read_b128 ahead of the MFMAs that use it; sched_barrier keeps hipcc from hoisting all
      // NG reads (4*NG VGPRs) to the loop top
      f32x4 a_cur = *reinterpret_cast<const f32x4*>(arow);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        f32x4 a_nxt = a_cur;
        if (g + 1 < NG) a_nxt = *reinterpret_cast<const f32x4*>(arow + 8 * (g + 1));
        f32x4 rg;
        if constexpr (RFL > 0) { if (g >= RFR) rg = rfl[(g - RFR) * 64]; else rg = rf[g < RFR ? g : 0]; } else rg = rf[g];
        X = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[0], rg[0], X, 0, 0, 0);
        X = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[1], rg[1], X, 0, 0, 0);
        X = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[2], rg[2], X, 0, 0, 0);
        X = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[3], rg[3], X, 0, 0, 0);
        a_cur = a_nxt;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    return X;
  };

  // ---- per-tile softmax math on the accumulator: statistics (FWD/RANK/FUSED) and the GEMM2 coefficients (BWD/FUSED) ----
  auto epilogue = [&](const float* T, int t, const f32x16& X, float (&coef)[16], auto full) {
    constexpr bool FULL = decltype(full)::value;
    const int64_t c0 = c_begin + 32 * (int64_t)t;
    // ---- per-column terms of this lane's 16 accumulator rows: c = c0 + 8*q + 4*h + i ----
    float ac[16], sc[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if constexpr (NO_AC) {
        // nothing staged: the bias store_tile would have staged for a null a_c - 0, or -big past the end - is applied below
      } else {
        const f32x4 va = *reinterpret_cast<const f32x4*>((ROW_LDS ? rowterm + 32 * t : T + TILE_F) + 8 * q + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) ac[4 * q + i] = va[i];
      }
      if constexpr (IS_BWD) {
        const f32x4 vs = *reinterpret_cast<const f32x4*>((ROW_LDS ? rowterm + kRowTermRows + 32 * t : T + TILE_F + 32) + 8 * q + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[4 * q + i] = vs[i];
      }
    }
    float hth[16];                                   // per-element hard-negative threshold: max(row's, column's)
    if constexpr (hn) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 vh = *reinterpret_cast<const f32x4*>(T + TILE_F + 128 + 8 * q + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) hth[4 * q + i] = fmaxf(vh[i], hr);
      }
    }
    // wave-uniform: does this tile hold the positive of any row of this wave?
    bool diag_tile;
    if constexpr (FAST) {
      diag_tile = t >= dt_lo && t <= dt_hi;
    } else if (p.pos_idx != nullptr) {
      const int64_t dd0 = cpos - c0;
      diag_tile = __any(dd0 >= 0 && dd0 < 32) != 0;
    } else {
      diag_tile = (c0 < r0w + p.diag + 32) && (c0 + 32 > r0w + p.diag);
    }
    // tile-local row (minus the lane half's +4h) of this lane's positive, or a value no row matches
    int dloc = -100;
    if (diag_tile) {
      if constexpr (FAST) {
        // (no range test: a positive outside the tile gives a value outside 0 .. 31 - 4h, which no accumulator row equals)
        dloc = lnh + (int)(dfrag_lo - 32u * (unsigned)t);
      } else {
        const int64_t dd = cpos - c0;
        dloc = (dd >= 0 && dd < 32) ? (int)dd - 4 * h : -100;
      }
    }
    // The positive pair's fix-ups under the wave-uniform `if (diag_tile)` are selects: an `if` per register was a tree of ~25
    // nested exec branches per tile step.  Except the capture of the positive logit in the kernels with accidental-hit ids:
    // there the selects cost 13-18 VGPRs (forward pass with ids 166 -> 179: 3 -> 2 waves per SIMD; bf16x3 with ids and hard
    // negatives 44 -> 104 B of scratch); with the branches kept those kernels need fewer registers than before (156; 8 B).
    auto take_pos = [&](bool hit, float v) {
      if constexpr (HAS_IDS) {
        if (hit) { pos = v; have_pos = true; }
      } else {
        pos = hit ? v : pos;
        have_pos = have_pos || hit;
      }
    };
    bool dup[16];
    if constexpr (HAS_IDS) {
      const int64_t* idc = reinterpret_cast<const int64_t*>(T + TILE_F + 64) + 4 * h;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        dup[reg] = (idc[tt::acc_row(reg, 0)] == idr) && (tt::acc_row(reg, 0) != dloc);
    }

    if constexpr (MODE == MODE_RANK) {
      // rank of the positive = number of OTHER columns scoring strictly above the row's threshold (its own logit)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float v = __builtin_fmaf(X[reg], p.c1, ac[reg]);
        bool above = v > ar && tt::acc_row(reg, 0) != dloc;
        if constexpr (HAS_IDS) above = above && !dup[reg];          // an accidental hit is not a competitor (tfrs: its logit is -inf)
        cnt += above ? 1 : 0;
      }
    } else if constexpr (MODE == MODE_FWD) {
      float t2[16];
      float mx = kNegBig;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        float v = __builtin_fmaf(X[reg], p.c1, ac[reg]);
        if constexpr (HAS_IDS) v = dup[reg] ? kNegBig : v;
        if constexpr (hn) v = (v < hth[reg] && tt::acc_row(reg, 0) != dloc) ? kNegBig : v;
        t2[reg] = v;
        mx = fmaxf(mx, v);
      }
      if (diag_tile) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) take_pos(tt::acc_row(reg, 0) == dloc, t2[reg]);
      }
      const float m_new = fmaxf(run_m, mx);
      float sum = 0.f;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) sum += __builtin_amdgcn_exp2f(t2[reg] - m_new);
      run_l = run_l * __builtin_amdgcn_exp2f(run_m - m_new) + sum;
      run_m = m_new;
    } else {
      if constexpr (IS_BWD) {
        float tvs[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) tvs[reg] = NO_ROW ? __builtin_fmaf(X[reg], p.c1, ac[reg]) : __builtin_fmaf(X[reg], p.c1, ac[reg]) + ar;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const float w = NO_ROW ? sc[reg] : sc[reg] * sr;
          float tv = tvs[reg];
          if constexpr (hn) tv = (tv < hth[reg] && tt::acc_row(reg, 0) != dloc) ? kNegBig : tv;
          float e = __builtin_amdgcn_exp2f(tv) * w;
          if constexpr (HAS_IDS) e = dup[reg] ? 0.f : e;
          coef[reg] = e;
        }
        if (diag_tile) {                            // (selects: an `if` per register was a tree of exec branches)
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            const float d = coef[reg] - (NO_ROW ? sc[reg] : sc[reg] * sr);
            coef[reg] = tt::acc_row(reg, 0) == dloc ? d : coef[reg];
          }
        }
      } else {
        // FUSED (flash-style): online softmax over c; coef = exp2(t - m_row) un-normalised, the accumulators
        // carry sum_c p*K[c] at scale m_row.  Both lane halves of a row share ONE running max (GEMM2 sums
        // over both halves' c).  Lazy rescale (threshold kRescaleThr): wave-uniform branch.
        float mx = kNegBig;
        float vs[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          if constexpr (NO_AC) {                      // fma(X, c1, 0) = X * c1; a row past the end: fma(X, c1, -big), as staged before
            const float v0 = X[reg] * p.c1;
            vs[reg] = (FULL || tt::acc_row(reg, 0) + 4 * h < ncols - 32 * t) ? v0 : __builtin_fmaf(X[reg], p.c1, kNegBig);
          } else {
            vs[reg] = __builtin_fmaf(X[reg], p.c1, ac[reg]);
          }
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          float v = vs[reg];
          if constexpr (HAS_IDS) v = dup[reg] ? kNegBig : v;
          if constexpr (hn) v = (v < hth[reg] && tt::acc_row(reg, 0) != dloc) ? kNegBig : v;
          coef[reg] = v;
          mx = fmaxf(mx, v);
        }
        if (diag_tile) {
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) take_pos(tt::acc_row(reg, 0) == dloc, coef[reg]);
        }
        if constexpr (FAST)      // (the other half's lane by its byte address, computed once: __shfl_xor rebuilds it on every tile)
          mx = fmaxf(mx, __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(xor32_addr, __builtin_bit_cast(int, mx))));
        else
          mx = fmaxf(mx, __shfl_xor(mx, 32));
        if (__any(mx - run_m > kRescaleThr)) {
          const float m_new = fmaxf(run_m, mx);
          const float alpha = __builtin_amdgcn_exp2f(run_m - m_new);
          run_l *= alpha;
#pragma unroll
          for (int b = 0; b < NBW; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) G[b][i] *= alpha;
          run_m = m_new;
        }
        // the sum of the 16 exponentials as two interleaved chains (even / odd registers), then the pair
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          coef[2 * q] = __builtin_amdgcn_exp2f(coef[2 * q] - run_m);
          coef[2 * q + 1] = __builtin_amdgcn_exp2f(coef[2 * q + 1] - run_m);
          s0 = q == 0 ? coef[0] : s0 + coef[2 * q];
          s1 = q == 0 ? coef[1] : s1 + coef[2 * q + 1];
        }
        run_l += s0 + s1;
      }
    }
  };

  // quarter_done(k) (WG and CW only, else unused): called behind the last read of the tile's rows 8k .. 8k+7
  auto gemm2 = [&](const float* T, const float (&coef)[16], auto quarter_done) {
    if constexpr (PREC == 1) {
      // ---- GEMM2 (bf16x3): G^T[d = 32 b + acc row][r] += sum_c K[c][d] * coef[c][r].  The accumulator's registers
      // 8s .. 8s+7 ARE the B fragment of k-step s (element j of lane half h = tile row c = 16s + 8(j>>2) + 4h + (j&3));
      // the A fragment K^T[d][those c] comes out of the SAME row-major images through transposing reads
      // (ds_read_b64_tr_b16: a 16-lane group fetches 4 rows x 16 columns and gets them column-major). ----
      bf16x8 c_hi[2], c_mid[2];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const __bf16 hi = (__bf16)coef[i];
        c_hi[i >> 3][i & 7] = hi;
        c_mid[i >> 3][i & 7] = (__bf16)(coef[i] - (float)hi);
      }
      const char* img = reinterpret_cast<const char*>(T);
      const int g16 = (lane >> 4) & 1, q = (lane >> 2) & 3, pp = lane & 3;
      // flat step i = 2 b + s; the four transposing reads of step i+1 are in flight under the three MFMAs of step i
      constexpr int NSTEP = 2 * NBW;
      auto frag = [&](int i, bf16x8& k_hi, bf16x8& k_mid) {
        const int b = i >> 1, s = i & 1;
        const int sub = (SPLIT ? hw : ((32 * b) >> 7)) * HALF_B + 8 * (pp & 1);     // (SPLIT: b counts inside the wave's own 128 columns)
        const int ch = (((32 * b) & 127) >> 3) + 2 * g16 + (pp >> 1);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int row = 16 * s + 8 * half + 4 * h + q;
          const int off = sub + img_off(row, ch);
          const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + off));
          const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + PIECE_B + off));
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            k_hi[4 * half + e] = __builtin_bit_cast(__bf16, (short)v0[e]);
            k_mid[4 * half + e] = __builtin_bit_cast(__bf16, (short)v1[e]);
          }
        }
      };
      bf16x8 k_hi, k_mid;
      frag(0, k_hi, k_mid);
#pragma unroll
      for (int i = 0; i < NSTEP; ++i) {
        bf16x8 n_hi = k_hi, n_mid = k_mid;
        if (i + 1 < NSTEP) frag(i + 1, n_hi, n_mid);
        const int b = i >> 1, s = i & 1;
        G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k_mid, c_hi[s], G[b], 0, 0, 0);
        G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k_hi, c_mid[s], G[b], 0, 0, 0);
        G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k_hi, c_hi[s], G[b], 0, 0, 0);
        k_hi = n_hi; k_mid = n_mid;
        __builtin_amdgcn_sched_barrier(0);
      }
      return;
    } else {
      // ---- GEMM2: G^T[d = NB*i + b][r] += K[c(reg,h)][d] * coef[reg] ----
      const float* kbase = T + 4 * h * LS + NB * ln;
      f32x4 kc0, kc1;
      auto read_k = [&](int reg, f32x4& k0, f32x4& k1) {
        const float* krow = kbase + tt::acc_row(reg, 0) * LS;
        if constexpr (NB == 8) {
          k0 = *reinterpret_cast<const f32x4*>(krow);
          k1 = *reinterpret_cast<const f32x4*>(krow + 4);
        } else if constexpr (NB == 4) {
          k0 = *reinterpret_cast<const f32x4*>(krow);
        } else if constexpr (NB == 2) {
          const float2 k2 = *reinterpret_cast<const float2*>(krow);
          k0[0] = k2.x; k0[1] = k2.y;
        } else {
          k0[0] = krow[0];
        }
      };
      read_k(0, kc0, kc1);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        f32x4 kn0 = kc0, kn1 = kc1;
        if (reg + 1 < 16) read_k(reg + 1, kn0, kn1);
#pragma unroll
        for (int b = 0; b < (NB < 4 ? NB : 4); ++b)
          G[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(kc0[b], coef[reg], G[b], 0, 0, 0);
        if constexpr (NB == 8) {
#pragma unroll
          for (int b = 0; b < 4; ++b)
            G[4 + b] = __builtin_amdgcn_mfma_f32_32x32x2f32(kc1[b], coef[reg], G[4 + b], 0, 0, 0);
        }
        kc0 = kn0; kc1 = kn1;
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (INWG) {
          // (the reads of step reg + 1 are already issued: they touch rows 8k + 8 and up, or nothing at all behind the last step)
          if ((reg & 3) == 3) {
            quarter_done(reg >> 2);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
  };
  auto no_hook = [](int) {};

  if constexpr (WG) {
    // ---- WG: GEMM1 -> epilogue -> GEMM2 per tile on the wave's private buffer, no barrier.  The chunk stream (load_chunk): behind
    // quarter k of tile t's GEMM2, chunk k of tile t + 1 is written and the chunk two further on - k + 2 of tile t + 1, or k - 2 of
    // tile t + 2 - requested into the same registers.  full: tiles t + 1 and t + 2 are full tiles, as t itself. ----
    auto wg_step = [&](int t, auto full) {
      constexpr bool FULL = decltype(full)::value;
      asm volatile("" ::: "memory");                   // (the wave reads back what its own lanes have written: program order)
      const f32x16 X = gemm1(TW);
      store_S(t, X);
      float coef[16];
      epilogue(TW, t, X, coef, full);
      gemm2(TW, coef, [&](int k) {
        asm volatile("" ::: "memory");
        store_chunk(ck[k & 1], t + 1, k, full);
        const int tn = k < 2 ? t + 1 : t + 2;
        load_chunk(ck[k & 1], FULL ? tn : clamp_tile(tn), (k + 2) & 3, full);
      });
    };
    // (prologue and loops under ONE test of the tile count: the loops are entered behind the prologue's full wait on every path)
    if (ntiles > 0) {
      // tile 0 whole, in one round trip (the gradient block is not live yet: registers for 16 float4), then the stream's first two
      // chunks, which belong to tile 1
      f32x4 t0a[2][4], t0b[2][4];
      load_chunk(t0a[0], 0, 0, GEN); load_chunk(t0a[1], 0, 1, GEN); load_chunk(t0b[0], 0, 2, GEN); load_chunk(t0b[1], 0, 3, GEN);
      // s_waitcnt vmcnt(0), written out: the fragment's loads above sit under the lane mask r_ok, so the compiler cannot count
      // them as issued, and without a full wait it knows of it put one in front of the fragment's first use - the first MFMA of
      // GEMM1, in every trip of the tile loops
      __builtin_amdgcn_s_waitcnt(0x0F70);
      store_chunk(t0a[0], 0, 0, GEN); store_chunk(t0a[1], 0, 1, GEN); store_chunk(t0b[0], 0, 2, GEN); store_chunk(t0b[1], 0, 3, GEN);
      load_chunk(ck[0], clamp_tile(1), 0, GEN);
      load_chunk(ck[1], clamp_tile(1), 1, GEN);
      int t = 0;
      const int nfast = nfull > 2 ? nfull - 2 : 0;
      for (; t < nfast; ++t) wg_step(t, FULL_TILE);
      for (; t < ntiles; ++t) wg_step(t, GEN);
    }
  } else if constexpr (CW) {
    // ---- CW: epilogue -> GEMM2 per tile on the stored dot products and the wave's private buffer, no barrier.  Every split is
    // ntiles >= 1 FULL tiles (launch_score checks), so there is one step form: no tail loop, no mask_S, no row clamp; only the tile
    // INDEX of a prefetch is clamped (a scalar minimum: past its split's end a wave reads its last tile again and nobody consumes
    // it).  Per step, in order of need: the dot products of tile t + 2 into the register set tile t has just left (full_step's
    // order), a_c / s_c of tile t + 1 (lane = row, both halves alike), then behind quarter k of GEMM2 chunk k of tile t + 1 is
    // written and the chunk two further on requested, as in WG; the row terms are written behind the last quarter. ----
    static_assert(kSPrefetch == 2, "two register sets of stored dot products");
    f32x16 xa, xb;
    float sd_a = 0.f, sd_s = 0.f;
    const unsigned sd_off = (unsigned)ln;
    auto load_side = [&](int t) {                      // t: a tile that exists
      sd_a = uniform_base(acp + 32 * (int64_t)t)[sd_off];
      sd_s = uniform_base(scp + 32 * (int64_t)t)[sd_off];
    };
    auto store_side = [&]() { TW[TILE_F + lane] = h ? sd_s : sd_a; };       // [a_c: 32 | s_c: 32]
    auto cw_step = [&](int t, f32x16& xs_t) {
      asm volatile("" ::: "memory");                   // (the wave reads back what its own lanes have written: program order)
      float coef[16];
      epilogue(TW, t, xs_t, coef, FULL_TILE);
      load_S(clamp_tile(t + 2), xs_t);
      load_side(clamp_tile(t + 1));
      gemm2(TW, coef, [&](int k) {
        asm volatile("" ::: "memory");
        store_chunk(ck[k & 1], t + 1, k, FULL_TILE);
        if (k == 3) store_side();
        load_chunk(ck[k & 1], clamp_tile(k < 2 ? t + 1 : t + 2), (k + 2) & 3, FULL_TILE);
      });
    };
    // tile 0 whole, in one round trip (the gradient block is not live yet: registers for 16 float4), behind the dot products of the
    // first two tiles; the stream's first two chunks, which belong to tile 1, are requested behind tile 0's write, so the loop is
    // entered with exactly what every trip leaves in flight: two chunks
    load_S(0, xa);
    load_S(clamp_tile(1), xb);
    f32x4 t0a[2][4], t0b[2][4];
    load_chunk(t0a[0], 0, 0, FULL_TILE); load_chunk(t0a[1], 0, 1, FULL_TILE);
    load_chunk(t0b[0], 0, 2, FULL_TILE); load_chunk(t0b[1], 0, 3, FULL_TILE);
    load_side(0);
    if (blockIdx.x == 0) {
      // loss = sum of the per-row losses pass 1 has written, by the first workgroup, under its first tile's round trip: exactly
      // sum_rows_kernel's order - 1024 strided partial sums (two per thread), then the binary tree, whose first step (s = 512) is the
      // sum of a thread's two.  Loads unconditional from clamped rows; the trip count is the workgroup's, not the thread's.
      float* red = smem + WAVES * WBUF_F;
      const int64_t nrow = p.n_c;
      float a0 = 0.f, a1 = 0.f;
      for (int64_t b0 = 0; b0 < nrow; b0 += 8 * 1024) {
        float v[8][2];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int64_t rr = b0 + 1024 * i + 512 * j + tid;
            v[i][j] = p.per_row[rr < nrow ? rr : nrow - 1];
          }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (b0 + 1024 * i + tid < nrow) a0 += v[i][0];
          if (b0 + 1024 * i + 512 + tid < nrow) a1 += v[i][1];
        }
      }
      red[tid] = a0 + a1;
      __syncthreads();
      static_assert(THREADS == 512, "a thread holds two of the 1024 partial sums");
      for (int s2 = 256; s2 > 0; s2 >>= 1) {
        if (tid < s2) red[tid] += red[tid + s2];
        __syncthreads();
      }
      if (tid == 0) p.loss[0] = red[0];
    }
    store_chunk(t0a[0], 0, 0, FULL_TILE); store_chunk(t0a[1], 0, 1, FULL_TILE);
    store_chunk(t0b[0], 0, 2, FULL_TILE); store_chunk(t0b[1], 0, 3, FULL_TILE);
    store_side();
    load_chunk(ck[0], clamp_tile(1), 0, FULL_TILE);
    load_chunk(ck[1], clamp_tile(1), 1, FULL_TILE);
    // whole pairs in the loop, an odd last tile behind it (see the slab form below)
    int t = 0;
    for (; t + 1 < ntiles; t += 2) {
      cw_step(t, xa);
      cw_step(t + 1, xb);
    }
    if (t < ntiles) cw_step(t, xa);
  } else if constexpr (FROM_S && kSPrefetch == 2) {
    // ---- BWD_S: epilogue -> GEMM2 per tile on the stored dot products; those of tiles t+1 AND t+2 are in flight while tile
    // t is worked on (two register sets, the body instantiated for each: f32 170 -> 168 us, bf16x3 96 -> 89 us) ----
    f32x16 xa, xb;
#pragma unroll
    for (int i = 0; i < 16; ++i) { xa[i] = 0.f; xb[i] = 0.f; }
    // Order of issue in a step = order of need: the staged tile (waited for at this step's store_tile, behind GEMM2), then the
    // dot products of tile t+2 (consumed two steps on) - so the wait in front of the ds_write leaves those 16 loads in flight.
    auto tile_step = [&](int t, f32x16& xs_t) {
      if constexpr (PREC == 1) load_tile(clamp_tile(t + 1), GEN);
      const float* T = smem + (t % NBUF) * BUF_F;
      const f32x16 X = mask_S(t, xs_t);
      float coef[16];
      epilogue(T, t, X, coef, GEN);
      if constexpr (PREC == 0) load_tile(clamp_tile(t + TPB), GEN);
      load_S(clamp_tile(t + 2), xs_t);
      gemm2(T, coef, no_hook);
      store_tile(t + TPB, (t + TPB) % NBUF, GEN);
      if ((t % TPB) == TPB - 1) __syncthreads();
    };
    // FAST: tiles t, t + TPB and t + 2 exist and are full (t + 2 < nfull) - the dot products are used as loaded, the loads and
    // the LDS store of tile t + TPB take no clamp and no select
    // rb = t % NBUF, carried by the loop: the two steps of a trip sit one buffer apart, so both take their LDS addresses from
    // the trip's one base (a compile-time offset apart) instead of each from its own t % NBUF
    auto full_step = [&](int t, int rb, int rn, f32x16& xs_t) {
      const float* T = smem + rb * BUF_F;
      float coef[16];
      epilogue(T, t, xs_t, coef, FULL_TILE);
      load_tile(t + TPB, FULL_TILE);
      load_S(t + 2, xs_t);
      gemm2(T, coef, no_hook);
      store_tile(t + TPB, rn, FULL_TILE);
      if ((t % TPB) == TPB - 1) __syncthreads();
    };
    if (ntiles > 0) {                                  // (an empty split issues nothing at all)
      load_S(0, xa);
      load_S(clamp_tile(1), xb);
      // whole pairs in the loop, an odd last tile behind it: with the second step of a pair under an `if`, the compiler has to
      // allow for a path on which its loads were never issued, and the wait for tile t at the top of the loop drains tile t+1 too
      int t = 0;
      if constexpr (FAST) {                            // whole pairs of steps whose tiles and prefetches are full tiles
        static_assert(TPB <= 2, "full_step prefetches at most two tiles ahead");
        static_assert(NBUF == 2 || NBUF == 4, "a trip of two steps starts at an even buffer");
        const int nfast = (nfull > 2 ? nfull - 2 : 0) & ~1;
        for (int rb = 0; t < nfast; t += 2, rb = (rb + 2) % NBUF) {
          const int rn = (rb + TPB) % NBUF;            // where tile t + TPB is staged; tile t + 1 + TPB goes one buffer further
          full_step(t, rb, rn, xa);
          full_step(t + 1, rb + 1, TPB == 2 ? rn + 1 : (rb + 1 + TPB) % NBUF, xb);
        }
      }
      for (; t + 1 < ntiles; t += 2) {
        tile_step(t, xa);
        tile_step(t + 1, xb);
      }
      if (t < ntiles) tile_step(t, xa);
    }
  } else {
    // ---- every wave runs GEMM1 -> epilogue -> GEMM2 per tile; 2 LDS buffers, one barrier per tile ----
    // History (r02 -> r03).  In r02 a build of this loop with its body in a lambda called twice per iteration (the form the
    // BWD_S branch above uses) gave, for score_kernel<256, FWD>, wrong values in about half the rows, different from run to
    // run; the note left here said its loop "exit test is a vector compare".  That build was never committed.  r03 rebuilt
    // the form from the description (TT_LOOP_LAMBDA=1, below) with the same compiler: its ISA has SCALAR loop control
    // (s_cmp / s_cbranch_scc on the tile count), the `s_waitcnt vmcnt(0)` in front of every staged tile's ds_write and
    // `s_waitcnt lgkmcnt(0)` in front of every s_barrier exactly as the plain loop, and it passes the parity and determinism
    // tests on the GPU three runs out of three (profiles/r03_loop_lambda_audit.txt) - so the lambda form as such is not the
    // cause.  What the r02 note does pin down is a trip count held in VGPRs: results that change from run to run need waves
    // that disagree about how often they reach the barrier, and the only way the tile loop gets there is a per-lane copy of
    // `ntiles` / `t` (the quotient blockIdx / nsplit is computed on the vector ALU) that the compiler no longer proves uniform
    // once the loop body is large enough to spill or re-materialise it (D = 256: 240+ VGPRs).  The fix is by construction:
    // split, row block and ntiles go through readfirstlane (top of the kernel), so in EVERY loop form the compiler sees
    // scalar control, and tests/isa_audit/audit_barriers.py verifies on the built ISA - for all 112 instantiations, both loop forms -
    // that each barrier loop closes and exits on scalar branches and that no barrier can be skipped under a lane mask (the
    // script's negative control, a barrier loop on a per-lane trip count, is flagged).  The shipping BWD_S loop above
    // satisfies the same condition.  tests: test_retrieval_baseline_configs[1024-256], test_retrieval_is_deterministic
    // (dims 128 and 256, every form, rank pass), test_retrieval_odd_and_short_tile_counts.
    f32x16 xs;
#pragma unroll
    for (int i = 0; i < 16; ++i) xs[i] = 0.f;
    if constexpr (FROM_S) { if (ntiles > 0) load_S(0, xs); }
    int t_first = 0;                                   // first tile of the general loop below
    if constexpr (FAST) {
      // MODE_FUSED_S_NC's main loop: tile t and the tile t + TPB it prefetches are full tiles (t + TPB < nfull)
      static_assert(!FROM_S && !SPLIT, "the fast form of pass 1");
      const int nfast = nfull > TPB ? nfull - TPB : 0;
      for (int t = 0; t < nfast; ++t) {
        const float* T = smem + (t % NBUF) * BUF_F;
        const f32x16 X = gemm1(T);
        store_S(t, X);
        float coef[16];
        epilogue(T, t, X, coef, FULL_TILE);
        load_tile(t + TPB, FULL_TILE);
        gemm2(T, coef, no_hook);
        store_tile(t + TPB, (t + TPB) % NBUF, FULL_TILE);
        if ((t % TPB) == TPB - 1) __syncthreads();
      }
      t_first = nfast;
    }
#if TT_LOOP_LAMBDA
    auto tile_step = [&](int t) {
      if constexpr (MODE == MODE_FWD || MODE == MODE_RANK || PREC == 1) load_tile(clamp_tile(t + 1), GEN);
      const float* T = smem + (t % NBUF) * BUF_F;
      f32x16 X;
      if constexpr (FROM_S) X = mask_S(t, xs); else X = gemm1(T);
      if constexpr (SPLIT) exchange(X);
      if constexpr (TO_S) store_S(t, X);
      float coef[16];
      epilogue(T, t, X, coef, GEN);
      if constexpr (IS_BWD || IS_FUSED) {
        if constexpr (PREC == 0) load_tile(clamp_tile(t + TPB), GEN);
        if constexpr (FROM_S) load_S(clamp_tile(t + 1), xs);
        gemm2(T, coef, no_hook);
      }
      store_tile(t + TPB, (t + TPB) % NBUF, GEN);
      if ((t % TPB) == TPB - 1) __syncthreads();
    };
    for (int t = t_first; t < ntiles; t += 2) {
      tile_step(t);
      if (t + 1 < ntiles) tile_step(t + 1);
    }
#else
    for (int t = t_first; t < ntiles; ++t) {
      // FWD/RANK: prefetch the next tile at the top.  BWD/FUSED: registers are tight (rf + G + X + coef), so the
      // prefetch is issued just before GEMM2, whose 16*NB MFMAs (>= 1.7 us at D=128) cover its latency.
      // bf16x3: a tile is ~1 us of MFMAs, less than a global round trip under load: the prefetch goes to the top too
      if constexpr (MODE == MODE_FWD || MODE == MODE_RANK || PREC == 1) load_tile(clamp_tile(t + 1), GEN);
      const float* T = smem + (t % NBUF) * BUF_F;
      f32x16 X;
      if constexpr (FROM_S) X = mask_S(t, xs); else X = gemm1(T);
      if constexpr (SPLIT) exchange(X);
      if constexpr (TO_S) store_S(t, X);
      float coef[16];
      epilogue(T, t, X, coef, GEN);
      if constexpr (IS_BWD || IS_FUSED) {
        if constexpr (PREC == 0) load_tile(clamp_tile(t + TPB), GEN);
        if constexpr (FROM_S) load_S(clamp_tile(t + 1), xs);                 // next tile's dot products, under GEMM2
        gemm2(T, coef, no_hook);
      }
      store_tile(t + TPB, (t + TPB) % NBUF, GEN);
      if ((t % TPB) == TPB - 1) __syncthreads();       // (uniform) tiles of the next group are complete, this group's buffers free
    }
#endif
  }

  // ---- epilogue ----
  if constexpr (WG) {
    // The 8 splits of the fragment's 32 rows meet in LDS: every wave leaves (run_m, L) per row behind the tile buffers and its
    // gradient block in its own tile buffer (dead by now; [32 rows][LS], the slab's row layout), the one wave that met a row's
    // positive its logit.  One barrier; then fused_combine_kernel's arithmetic (combine_row) on 32 float4 lanes per row, two
    // (row, lane) pairs per thread.  The positive's row of K and the sample weight are requested in front of the barrier.
    float* stat = smem + WAVES * TILE_F;               // [m: 8 x 32 | l: 8 x 32 | positive logit: 32]
    const float L = run_l + __shfl_xor(run_l, 32);      // both halves share run_m
    asm volatile("" ::: "memory");
    if (h == 0) {
      stat[wave * 32 + ln] = run_m;
      stat[WAVES * 32 + wave * 32 + ln] = L;
    }
    if (have_pos) stat[2 * WAVES * 32 + ln] = pos;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int i = tt::acc_row(reg, 0) + 4 * h;        // G[b][reg] = G^T[d = NB * i + b][r = ln], NB == 4
      *reinterpret_cast<f32x4*>(TW + ln * LS + 4 * i) = f32x4{G[0][reg], G[1][reg], G[2][reg], G[3][reg]};
    }
    const int c4 = tid & 31;
    int64_t crow[2];
    f32x4 cp[2];
    float wr[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      crow[j] = r0w + (tid >> 5) + 16 * j;
      const int64_t rc = crow[j] < p.n_r ? crow[j] : p.n_r - 1;
      cp[j] = reinterpret_cast<const f32x4*>(p.K + (rc + p.diag) * D)[c4];
      wr[j] = p.w != nullptr ? p.w[rc] : 1.0f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int rl = (tid >> 5) + 16 * j;              // the row within the fragment
      const int64_t row = crow[j];
      if (row < p.n_r)
        combine_row(WAVES, [&](int s) { return stat[s * 32 + rl]; }, [&](int s) { return stat[WAVES * 32 + s * 32 + rl]; },
                    [&](int s) { return *reinterpret_cast<const f32x4*>(smem + s * TILE_F + rl * LS + 4 * c4); }, cp[j],
                    stat[2 * WAVES * 32 + rl], wr[j], p.scale, c4 == 0, p.lse + row, p.per_row + row, p.aq + row, p.sq + row,
                    reinterpret_cast<f32x4*>(p.dq + row * D) + c4);
    }
    return;
  }
  if constexpr (CW) {
    // The 8 splits of the fragment's 32 rows meet in LDS: every wave leaves its gradient block in its own tile buffer (dead by now;
    // [32 rows][LS], the slab's row layout).  One barrier; then reduce_slabs_kernel's sum - a = s0; a += s1; ... s7 - on 32 float4
    // lanes per row, two (row, lane) pairs per thread, stored as 16 bytes per lane.  Rows past n_r are dropped here.
    asm volatile("" ::: "memory");
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int i = tt::acc_row(reg, 0) + 4 * h;        // G[b][reg] = G^T[d = NB * i + b][r = ln], NB == 4
      *reinterpret_cast<f32x4*>(TW + ln * LS + 4 * i) = f32x4{G[0][reg], G[1][reg], G[2][reg], G[3][reg]};
    }
    __syncthreads();
    const int c4 = tid & 31;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int rl = (tid >> 5) + 16 * j;              // the row within the fragment
      const int64_t row = r0w + rl;
      f32x4 a = *reinterpret_cast<const f32x4*>(smem + rl * LS + 4 * c4);
#pragma unroll
      for (int s = 1; s < WAVES; ++s) a += *reinterpret_cast<const f32x4*>(smem + s * WBUF_F + rl * LS + 4 * c4);
      if (row < p.n_r) reinterpret_cast<f32x4*>(p.dr + row * D)[c4] = a;
    }
    return;
  }
  if constexpr (IS_FUSED) {
    const float L = run_l + __shfl_xor(run_l, 32);      // both halves share run_m
    if (r_ok && hw == 0) {
      if (h == 0) {
        p.part_m[(int64_t)split * p.n_r + r] = run_m;
        p.part_l[(int64_t)split * p.n_r + r] = L;
      }
      if (have_pos) p.pos2[r] = pos;
    }
  }
  if constexpr (MODE == MODE_RANK) {
    const int total = cnt + __shfl_xor(cnt, 32);
    if (r_ok && h == 0) p.part_cnt[(int64_t)split * p.n_r + r] = total;
  } else if constexpr (MODE == MODE_FWD) {
    const float om = __shfl_xor(run_m, 32);
    const float ol = __shfl_xor(run_l, 32);
    const float M = fmaxf(run_m, om);
    const float L = run_l * __builtin_amdgcn_exp2f(run_m - M) + ol * __builtin_amdgcn_exp2f(om - M);
    if (r_ok) {
      if (h == 0) {
        p.part_m[(int64_t)split * p.n_r + r] = M;
        p.part_l[(int64_t)split * p.n_r + r] = L;
      }
      if (have_pos) p.pos2[r] = pos;
    }
  } else {
    if (r_ok) {
      float* out = p.slab + ((int64_t)split * p.n_r + r) * D + 128 * hw;
      if constexpr (PREC == 1) {          // G[b][reg] = G^T[d = 32 b + acc row(reg, h)][r]: registers 4g .. 4g+3 are 4 consecutive d
#pragma unroll
        for (int b = 0; b < NBW; ++b)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *reinterpret_cast<f32x4*>(out + 32 * b + 8 * g + 4 * h) = f32x4{G[b][4 * g], G[b][4 * g + 1], G[b][4 * g + 2], G[b][4 * g + 3]};
      } else
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int i = tt::acc_row(reg, 0) + 4 * h;
        if constexpr (NB == 8) {
          *reinterpret_cast<f32x4*>(out + 8 * i) = f32x4{G[0][reg], G[1][reg], G[2][reg], G[3][reg]};
          *reinterpret_cast<f32x4*>(out + 8 * i + 4) = f32x4{G[4][reg], G[5][reg], G[6][reg], G[7][reg]};
        } else if constexpr (NB == 4) {
          *reinterpret_cast<f32x4*>(out + 4 * i) = f32x4{G[0][reg], G[1][reg], G[2][reg], G[3][reg]};
        } else if constexpr (NB == 2) {
          *reinterpret_cast<float2*>(out + 2 * i) = float2{G[0][reg], G[1][reg]};
        } else {
          out[i] = G[0][reg];
        }
      }
    }
  }
