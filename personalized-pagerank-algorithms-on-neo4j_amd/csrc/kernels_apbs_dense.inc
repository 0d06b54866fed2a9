// kernels_apbs_dense.inc — the dense tier's kernel (kernels_apbs.hip, "tier 2"), included once per in-edge record type:
// APBS_DENSE_KERNEL is the kernel's name, APBS_DENSE_REC its record type (InRec: k_apbs_dense, InRecW: k_apbs_dense_w).
// The helpers (dn_edge_range, dn_chunk, dn_help_once) are templates on the record; the kernel itself is stamped out
// under a plain name per type, because the profiles' per-kernel rows are keyed by "k_apbs_dense".
__global__ __launch_bounds__(kDnThreads) void APBS_DENSE_KERNEL(const int32_t* __restrict__ target_list, uint32_t n_targets,
                                                                 unsigned long long* next_target,
                                                                 const uint32_t* __restrict__ in_rp,
                                                                 const APBS_DENSE_REC* __restrict__ in_rec,
                                                                 const int32_t* __restrict__ old2new,
                                                                 const int32_t* __restrict__ new2old, double alpha,
                                                                 double rmax, ApOut O, char* ws_base, DnBoard* board,
                                                                 unsigned long long* done_targets,
                                                                 unsigned long long* n_open,
                                                                 unsigned long long* abort_word, DnDims D, int share,
                                                                 uint32_t n_owners, uint32_t hot_n, int help_between,
                                                                 unsigned long long* __restrict__ dbg) {
  // n_owners: the workgroups 0 .. n_owners - 1 have a workspace and take targets; the others only help with posted
  // levels (the pass for the few searches whose lists need room for every node: a handful of full-size workspaces,
  // the whole chip working on their levels)
  // dbg (developer switch PPRHIP_APBS_DEBUG, else nullptr; HOST memory): per workgroup {searches, edges of its own
  // searches, ticks of the 100 MHz clock spent in pops + scans, own edges, waiting for helpers, emission, clean-up,
  // helping / idle, the tick at which the workgroup ended, and where it is: stage << 32 | detail (printed by the
  // host's watchdog when a launch does not come back)}
  // hot_n: ids below it keep residue and reserve in this workgroup's LDS while it owns a search (dn_edge_range);
  // dynamic LDS: hres[hot_n], hrsv[hot_n]
  extern __shared__ double dn_hot[];
  double* const hres = dn_hot;
  double* const hrsv = dn_hot + hot_n;
  __shared__ DnLds L;
  __shared__ uint32_t s_scan[kDnWaves];
  __shared__ unsigned long long s_scan64[kDnWaves];
  __shared__ uint32_t s_pcount, s_carry, s_job[4], s_gaveup;
  __shared__ DnHelpLds H;
  __shared__ uint32_t s_tcount, s_nnext, s_giveup;  // the search's append counters while it stays on this workgroup
  __shared__ unsigned long long s_t, s_out_base, s_tot;
  const int tid = threadIdx.x;
  const uint32_t n = D.n, cap_t = D.cap_t, cap_f = D.cap_f, chunk = D.chunk;
  const DenseWs W = dense_ws_of(ws_base, blockIdx.x, D);
  DnBoard* B = board + blockIdx.x;
  const DnSinks S_local{&s_tcount, &s_nnext, &s_giveup};
  unsigned long long pops = 0, edges = 0;
  unsigned long long tk[6] = {0, 0, 0, 0, 0, 0}, t_mark = dbg ? wall_clock64() : 0ull, n_search = 0;
#define DN_TICK(i)                                   \
  if (dbg && tid == 0) {                             \
    const unsigned long long now_ = wall_clock64();  \
    tk[i] += now_ - t_mark;                          \
    t_mark = now_;                                   \
  }
#define DN_AT(stage, detail)                                                                                  \
  if (dbg && tid == 0)                                                                                        \
    __hip_atomic_store(dbg + (size_t)blockIdx.x * 12 + 9, ((unsigned long long)(stage) << 32) | (uint32_t)(detail), \
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  uint32_t seq = 0;  // even: this workgroup's board entry is closed
  for (uint32_t i = tid; i < 2 * hot_n; i += kDnThreads) dn_hot[i] = 0.0;
  __syncthreads();

  for (;;) {
    if (blockIdx.x >= n_owners) break;
    if (tid == 0) s_t = atomic_add_u64(next_target, 1ull);
    __syncthreads();
    const unsigned long long ti = s_t;
    if (ti >= n_targets) break;
    n_search++;
    DN_AT(1, ti)
    const int32_t t_old = target_list[ti];
    const int32_t t = old2new[t_old];
    uint32_t nf = 0, which = 0;
    if (tid == 0) {
      // the record buffer is full: not run, listed for the host's next pass (see the LDS tier)
      s_job[1] = (__hip_atomic_load(O.out_valid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ~0ull) ? 1u : 0u;
      if (s_job[1]) {
        O.overflow_list[atomic_add_u64(O.overflow_count, 1ull)] = -(t_old + 1);
        atomic_add_u64(done_targets, 1ull);
      }
    }
    __syncthreads();
    if (s_job[1]) {
      __syncthreads();
      continue;
    }
    if (tid == 0) {
      s_pcount = 0;
      s_tcount = 0;
      s_giveup = 0;
      const bool hot_t = (uint32_t)t < hot_n;
      if (in_rp[t + 1] == in_rp[t]) {  // Backward_Search.java:46-49: reserve = {t: 1.0}
        if (hot_t) hrsv[t] = 1.0;
        else dn_store(&W.rsv[t], 1.0);
        dn_store(&W.plist[0], t);
        s_pcount = 1;
      } else {
        if (hot_t) {
          hres[t] = 1.0;  // :54-56; the target is pushed unconditionally first
        } else {
          dn_store(&W.res[t], 1.0);
          dn_store(&W.touched[0], t);
          s_tcount = 1;
        }
        dn_store(&W.fr[0][0], t);
        nf = 1;
      }
      s_job[0] = nf;
    }
    __syncthreads();
    nf = s_job[0];

    while (nf > 0) {
      // ---- every frontier node gives up its residue (:58-67,72; a node is in a level's frontier at most once) and
      // the level's edge space is laid out, a tile of kDnStage frontier entries at a time: pending contribution, first
      // in-edge, exclusive prefix of the in-degrees.  A level of one tile stays in LDS; a larger one (or one whose
      // edges are worth sharing) is written to the workspace, with the frontier position every chunk of edges starts in.
      const int32_t* cur = W.fr[which];
      const bool one_tile = nf <= (uint32_t)kDnStage;
      DN_AT(2, nf)
      if (tid == 0) {
        s_carry = 0;
        s_nnext = 0;
      }
      __syncthreads();
      for (uint32_t tile = 0; tile < nf; tile += kDnThreads) {
        const uint32_t i = tile + tid;
        uint32_t d = 0, b = 0;
        double pc = 0.0;
        if (i < nf) {
          const int32_t v = dn_load(&cur[i]);
          double rc;
          if ((uint32_t)v < hot_n) {  // (a node is in a level's frontier once: plain LDS accesses)
            rc = hres[v];
            hres[v] = 0.0;
            const double r0 = hrsv[v];
            if (r0 == 0.0) {  // first pop: listed like a cold node (emission and clean-up walk the list)
              const uint32_t pp = atomicAdd(&s_pcount, 1u);
              if (pp < cap_f) dn_store(&W.plist[pp], v);
              else s_giveup = 1;
            }
            hrsv[v] = r0 + rc * alpha;
          } else {
            rc = __hip_atomic_exchange(&W.res[v], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double r0 = dn_load(&W.rsv[v]);
            if (r0 == 0.0) {  // first pop of this node (alpha * rc > 0 ever after)
              const uint32_t pp = atomicAdd(&s_pcount, 1u);
              if (pp < cap_f) dn_store(&W.plist[pp], v);
              else s_giveup = 1;
            }
            dn_store(&W.rsv[v], r0 + rc * alpha);
          }
          pc = (1.0 - alpha) * rc;
          b = in_rp[v];
          d = in_rp[v + 1] - b;
        }
        uint32_t tile_tot = 0;
        const uint32_t ex = s_carry + block_excl_scan_n<uint32_t, kDnWaves>(d, s_scan, &tile_tot);
        if (one_tile) {  // (tile == 0)
          if (i < nf) {
            L.eoff[tid] = ex;
            L.row[tid] = b;
            L.c[tid] = pc;
          }
        } else if (i < nf) {
          dn_store(&W.pend[i], pc);
          dn_store(&W.frow[i], b);
          dn_store(&W.eoff[i], ex);
          if (d) {  // chunks whose first edge lies in this node's range start here
            const uint32_t c_lo = (uint32_t)(((unsigned long long)ex + chunk - 1) / chunk);
            const uint32_t c_hi = (uint32_t)(((unsigned long long)ex + d - 1) / chunk);
            for (uint32_t c = c_lo; c <= c_hi; ++c) dn_store(&W.cstart[c], i);
          }
        }
        __syncthreads();
        if (tid == 0) s_carry += tile_tot;
        __syncthreads();
      }
      const uint32_t E = s_carry;
      const uint32_t n_chunks = (uint32_t)(((unsigned long long)E + chunk - 1) / chunk);
      const bool post = !one_tile || (share && n_chunks >= kDnShareMin);
      pops += (tid == 0) ? nf : 0;
      edges += (tid == 0) ? E : 0;
      if (!post) {
        // ---- the level stays here: edges straight from the LDS tile, appends counted in LDS
        if (tid == 0) L.eoff[nf] = E;
        __syncthreads();
        DN_TICK(0)
        DN_AT(5, E)
        dn_edge_range<false>(W, L, nf, 0u, E, W.fr[which ^ 1], S_local, in_rec, rmax, cap_t, cap_f, hres, hot_n);
        dn_barrier_global();  // the appends have arrived before the next level reads them
        DN_TICK(1)
        if (tid == 0) {
          s_gaveup = (s_giveup || dn_load(abort_word)) ? 1u : 0u;
          s_job[0] = s_gaveup ? 0u : s_nnext;
        }
      } else {
        // ---- the level goes through the workspace: a one-tile level is written out first
        if (one_tile && (uint32_t)tid < nf) {
          const uint32_t ex = L.eoff[tid], nx = (uint32_t)tid + 1 < nf ? L.eoff[tid + 1] : E;
          dn_store(&W.pend[tid], L.c[tid]);
          dn_store(&W.frow[tid], L.row[tid]);
          dn_store(&W.eoff[tid], ex);
          if (nx > ex) {
            const uint32_t c_lo = (uint32_t)(((unsigned long long)ex + chunk - 1) / chunk);
            const uint32_t c_hi = (uint32_t)(((unsigned long long)nx - 1) / chunk);
            for (uint32_t c = c_lo; c <= c_hi; ++c) dn_store(&W.cstart[c], (uint32_t)tid);
          }
        }
        dn_hot_spill(W, hres, hot_n);  // helpers reach the hot residues through the global vector only
        if (tid == 0) {
          dn_store(&W.eoff[nf], E);
          // the appends of a posted level are counted on the board entry (helpers add to them)
          dn_reset(&B->tcount, s_tcount);
          dn_reset(&B->nnext, 0u);
          dn_reset(&B->giveup, s_giveup);
        }
        dn_barrier_global();  // the level's layout has arrived in memory before it is posted or read
        DN_TICK(0)
        // post the level; take chunks of it like any helper; go on when all of them are done
        if (tid == 0) {
          dn_store(&B->n_chunks, n_chunks);
          dn_store(&B->nf, nf);
          dn_store(&B->which, which);
          dn_reset(&B->done, 0u);  // (includes the release fence for the stores above)
          seq += 1;                // odd: open
          dn_reset(&B->next, (unsigned long long)seq << 32);
          if (share) atomic_add_u64(n_open, 1ull);  // what idle workgroups poll
          s_job[0] = (uint32_t)atomic_add_u64(&B->next, 1ull);  // first chunk (only helpers need the compare-and-swap)
        }
        __syncthreads();
        // NOTE on the shape of this loop (and of every loop in this kernel that holds barriers): a block that only
        // lane 0 executes must never be the last thing before the back edge while another such block opens the loop -
        // the compiler then threads the two together, lanes other than 0 loop back to the barrier on a path of their
        // own, and the waves pass it before lane 0 has written what they are about to read (seen in the ISA of an
        // earlier form of this loop: every wave re-read chunk 0 for ever).  Lane-0 blocks are followed by a barrier.
        for (uint32_t c = s_job[0]; c < n_chunks; c = s_job[0]) {
          __syncthreads();  // s_job[0] has been read by every wave
          DN_AT(3, c)
          dn_chunk(W, B, which, nf, E, c, in_rec, rmax, D, L, hot_n);
          if (tid == 0) {  // (dn_chunk ended with every wave's stores acknowledged)
            atomicAdd(&B->done, 1u);
            s_job[0] = (uint32_t)atomic_add_u64(&B->next, 1ull);
          }
          __syncthreads();
        }
        __syncthreads();
        DN_TICK(1)
        if (tid == 0) {
          // bounded: a wait that outlasts kDnWaitTicks (a bug, or a helper lost to a fault) raises the launch's abort
          // word, on which every loop of every workgroup ends; the host turns it into an error
          DN_AT(4, n_chunks)
          const unsigned long long t_wait = wall_clock64();
          while (dn_load(&B->done) < n_chunks && !dn_load(abort_word)) {
            __builtin_amdgcn_s_sleep(8);
            if (wall_clock64() - t_wait > kDnWaitTicks) atomic_add_u64(abort_word, 1ull);
          }
          seq += 1;  // even: closed (a helper's compare-and-swap on the old sequence fails from here on)
          dn_reset(&B->next, (unsigned long long)seq << 32);
          if (share) atomic_add_u64(n_open, ~0ull);
          s_tcount = dn_load(&B->tcount);
          s_giveup = dn_load(&B->giveup);
          s_gaveup = (s_giveup || dn_load(abort_word)) ? 1u : 0u;
          s_job[0] = s_gaveup ? 0u : dn_load(&B->nnext);
        }
        __syncthreads();
        dn_hot_fill(W, hres, hot_n);  // the level is closed: hot residues back into LDS, the vector's head zero again
        dn_barrier_global();
        DN_TICK(2)
      }
      __syncthreads();
      nf = s_job[0];
      which ^= 1;
      __syncthreads();
    }

    DN_AT(6, 0)
    // a list is full (or the launch is being aborted): the search goes to the whole-vector tier
    if (tid == 0) s_gaveup = (s_giveup || dn_load(abort_word)) ? 1u : 0u;
    __syncthreads();
    const bool gave_up = s_gaveup != 0;
    const uint32_t np = s_pcount < cap_f ? s_pcount : cap_f;
    // ---- emit entries >= threshold (Base_Whole_Graph.java:80-88): only popped nodes hold a reserve
    bool retry = gave_up;
    // Round 5: a search of up to kDnEmitRegs * 1024 pops (all but the hubs') reads its reserves ONCE: they stay in
    // registers between the count and the emission, and the cleared value goes back in the same walk - the count
    // pass, the emission pass and the clean-up's pass over the pop list were three gathers of the same scattered
    // entries (emission 6 % + clean-up 15 % of the tier's workgroup time, profiles/r05_apbs_summary.md).
    constexpr int kDnEmitRegs = 4;
    bool rsv_cleared = false;
    if (!gave_up && np <= (uint32_t)kDnEmitRegs * kDnThreads) {
      int32_t pv[kDnEmitRegs];
      double pr[kDnEmitRegs];
      unsigned long long run = 0;
#pragma unroll
      for (int j = 0; j < kDnEmitRegs; ++j) {
        const uint32_t i = (uint32_t)j * kDnThreads + tid;
        pv[j] = i < np ? dn_load(&W.plist[i]) : -1;
      }
#pragma unroll
      for (int j = 0; j < kDnEmitRegs; ++j) {
        pr[j] = 0.0;
        if (pv[j] >= 0) {
          if ((uint32_t)pv[j] < hot_n) {
            pr[j] = hrsv[pv[j]];
            hrsv[pv[j]] = 0.0;
          } else {
            pr[j] = dn_load(&W.rsv[pv[j]]);
          }
        }
        run += (pr[j] > 0.0 && pr[j] >= rmax) ? 1ull : 0ull;
      }
#pragma unroll
      for (int j = 0; j < kDnEmitRegs; ++j)
        if (pv[j] >= 0 && (uint32_t)pv[j] >= hot_n) dn_store(&W.rsv[pv[j]], 0.0);  // (a node is popped-listed once)
      rsv_cleared = true;
      const unsigned long long total = block_sum_u64(run, s_scan64);  // valid in thread 0
      if (tid == 0) {
        s_tot = total;
        s_out_base = total ? atomic_add_u64(O.out_count, total) : 0ull;
      }
      __syncthreads();
      const unsigned long long tot = s_tot;
      if (s_out_base + tot > O.out_cap) {
        retry = true;  // the triple buffer is full: the host drains it and runs this target again
        if (tid == 0) atomicMin(O.out_valid, s_out_base);
      } else if (tot) {
        unsigned long long at = s_out_base;
#pragma unroll
        for (int j = 0; j < kDnEmitRegs; ++j) {
          if ((uint32_t)j * kDnThreads >= np) break;  // (uniform)
          const bool take = pr[j] > 0.0 && pr[j] >= rmax;
          unsigned long long chunk_total = 0;
          const unsigned long long ex2 =
              block_excl_scan_n<unsigned long long, kDnWaves>(take ? 1ull : 0ull, s_scan64, &chunk_total);
          if (take) O.out_rec[at + ex2] = TripleRec{new2old[pv[j]], t_old, pr[j]};
          at += chunk_total;
        }
      }
    } else if (!gave_up) {
      // (a popped hot id's reserve is in LDS)
      unsigned long long run = 0;
      for (uint32_t c0 = 0; c0 < np; c0 += kDnThreads) {
        const uint32_t i = c0 + tid;
        double r = 0.0;
        if (i < np) {
          const int32_t v = dn_load(&W.plist[i]);
          r = (uint32_t)v < hot_n ? hrsv[v] : dn_load(&W.rsv[v]);
        }
        run += (r > 0.0 && r >= rmax) ? 1ull : 0ull;
      }
      const unsigned long long total = block_sum_u64(run, s_scan64);  // valid in thread 0
      if (tid == 0) {
        s_tot = total;
        s_out_base = total ? atomic_add_u64(O.out_count, total) : 0ull;
      }
      __syncthreads();
      const unsigned long long tot = s_tot;
      if (s_out_base + tot > O.out_cap) {
        retry = true;  // the triple buffer is full: the host drains it and runs this target again
        if (tid == 0) atomicMin(O.out_valid, s_out_base);
      } else {
        unsigned long long at = s_out_base;
        for (uint32_t c0 = 0; c0 < np; c0 += kDnThreads) {
          const uint32_t i = c0 + tid;
          const int32_t v = i < np ? dn_load(&W.plist[i]) : 0;
          double r = 0.0;
          if (i < np) {  // read for the last time: the cleared value goes back in the same walk
            if ((uint32_t)v < hot_n) {
              r = hrsv[v];
              hrsv[v] = 0.0;
            } else {
              r = dn_load(&W.rsv[v]);
              dn_store(&W.rsv[v], 0.0);
            }
          }
          const bool take = r > 0.0 && r >= rmax;
          unsigned long long chunk_total = 0;
          const unsigned long long ex2 =
              block_excl_scan_n<unsigned long long, kDnWaves>(take ? 1ull : 0ull, s_scan64, &chunk_total);
          if (take) {
            O.out_rec[at + ex2] = TripleRec{new2old[v], t_old, r};
          }
          at += chunk_total;
        }
        rsv_cleared = true;
      }
    }
    if (retry && tid == 0) {  // lists full: +t, triple buffer full: -(t + 1)
      const unsigned long long p = atomic_add_u64(O.overflow_count, 1ull);
      O.overflow_list[p] = gave_up ? t_old : -(t_old + 1);
    }
    __syncthreads();
    DN_TICK(3)
    DN_AT(7, 0)
    // ---- hand the vectors back all-zero (the hot ids' state: LDS; the head of the global vector is zero already)
    for (uint32_t i = tid; i < hot_n; i += kDnThreads) hres[i] = 0.0;  // (what the last level left below the threshold)
    if (!rsv_cleared) {
      for (uint32_t i = tid; i < np; i += kDnThreads) {
        const int32_t v = dn_load(&W.plist[i]);
        if ((uint32_t)v < hot_n) hrsv[v] = 0.0;
        else dn_store(&W.rsv[v], 0.0);
      }
    }
    const uint32_t nt = s_tcount;
    if (nt <= cap_t && s_pcount <= cap_f) {
      // (tried in round 5: eight lanes per listed node zeroing the 64 aligned bytes around it, so that the memory side
      // sees whole 64-byte writes - 545 / 512 ms against 563 / 527 ms for R-MAT 22's tier, 1 668 / 1 643 against 1 646 /
      // 1 618 ms for R-MAT 24's on the same box: no difference beyond the noise; the 8-byte stores stay)
      for (uint32_t i = tid; i < nt; i += kDnThreads) dn_store(&W.res[dn_load(&W.touched[i])], 0.0);
    } else {  // a list overflowed: clear everything
      for (uint32_t i = tid; i < n; i += kDnThreads) {
        dn_store(&W.res[i], 0.0);
        dn_store(&W.rsv[i], 0.0);
      }
      for (uint32_t i = tid; i < hot_n; i += kDnThreads) hrsv[i] = 0.0;
    }
    dn_barrier_global();  // the zeros have arrived before the next search's atomics can meet them
    if (tid == 0) atomic_add_u64(done_targets, 1ull);
    DN_TICK(4)
    __syncthreads();  // (lane-0 blocks never sit next to a back edge: see the note at the chunk loop)
    // ---- between two searches of its own the workgroup holds no state: in a short pass (launch_apbs) levels that are
    // open on other workgroups' boards come first.  The targets are taken largest first, so the open levels belong to
    // the searches the launch will end with; pushed early they are not what everybody waits for at the end.
    if (share && help_between) {
      DN_AT(8, 2)
      while (dn_help_once(H, L, board, ws_base, D, in_rec, rmax, hot_n, n_owners, n_open, done_targets, n_targets,
                          abort_word) != 0) {
      }
      DN_TICK(5)
    }
  }

  // ---- out of targets: help with posted levels until every target of the launch is finished
  if (share) {
    const unsigned long long t_idle = wall_clock64();
    DN_AT(8, 0)
    for (;;) {
      if (tid == 0 && wall_clock64() - t_idle > 4 * kDnWaitTicks) atomic_add_u64(abort_word, 1ull);
      const int r = dn_help_once(H, L, board, ws_base, D, in_rec, rmax, hot_n, n_owners, n_open, done_targets, n_targets,
                                 abort_word);
      if (r != 0) continue;  // pushed a chunk, or lost one to somebody faster: look again at once
      if (H.done) break;
      __syncthreads();  // (H.done has been read by every wave before lane 0 writes it again)
      for (int k = 0; k < 4; ++k) __builtin_amdgcn_s_sleep(127);  // ~15 us between polls
    }
    DN_TICK(5)
  }
  DN_AT(10, 0)
#undef DN_TICK
#undef DN_AT
  const unsigned long long ps = block_sum_u64(pops, s_scan64);
  const unsigned long long es = block_sum_u64(edges, s_scan64);
  if (tid == 0) {
    if (ps) atomic_add_u64(O.stat_pops, ps);
    if (es) atomic_add_u64(O.stat_edges, es);
    if (dbg) {
      unsigned long long* d = dbg + (size_t)blockIdx.x * 12;
      d[0] = n_search;
      d[1] = edges;
      for (int i = 0; i < 6; ++i) d[2 + i] = tk[i];
      d[8] = wall_clock64();
    }
  }
}
