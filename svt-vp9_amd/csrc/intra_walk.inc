/* intra_walk.inc -- THE wavefront walk of an intra picture, as text: the one body of svt_intra_kernel (intra_kernel.hip) and
 * svt_intra_rc_kernel (intra_recon_kernel.hip) from the worker's first statement to the end of its ticket loop.  The ticket draw,
 * svt_intra_cell_of_ticket, the 32x32 rule, the two flag waits, the unit loop with its malformed-grid checks, the drain and the flag
 * publication stand here and nowhere else: a visibility or deadlock fix is made once.
 *
 * Text, not a function template: both kernels are held at 128 VGPRs and spill, and the order in which the compiler inlines decides
 * their register allocation -- every template form that was compiled changed the scratch of one kernel or both (DESIGN.md 5.5), while
 * this form gives each kernel the assembly it had with the walk written out in its own file.
 *
 * MAY BE INCLUDED ONLY INSIDE A KERNEL BODY (a __global__ function launched as ceil(n_workers / INTRA_W) workgroups of 64 * INTRA_W
 * threads), as its first statements.  Expects in scope:
 *   P          const intra_pic_dev, the picture (intra_core.h)
 *   n_workers  int, the number of 64-lane workers of the launch
 *   INTRA_WALK_BLOCK(N, plane, x0, y0, mode, sb, have_right)
 *              a macro the including file defines just before the include and #undefs after it: an int expression, the (wave-uniform)
 *              eob of the N x N block of `plane` at sample (x0, y0) that it has just coded in the worker's slice of s_lds
 *   INTRA_WALK_PROF (optional)
 *              defined by the including file when it wants the -DINTRA_PROF timers of the walk (it then provides g_intra_fine[]); a
 *              kernel that does not define it compiles to the same code with and without -DINTRA_PROF
 * Declares: W, s_lds (the workgroup's LDS: W slices of INTRA_SLICE_DW dwords), wave, lane, c_cols, c_rows, n_cell; returns from the
 * kernel for a worker beyond n_workers; falls out of its loop, the wave converged, when the tickets have run out -- what the including
 * kernel writes behind the include runs once per worker then.
 * -DINTRA_FENCES selects the release / acquire form of the publication (intra_core.h). */
    constexpr int W = INTRA_W;
    __shared__ int32_t s_lds[W * INTRA_SLICE_DW];
    /* the worker: wave-uniform, and known to be so (readfirstlane) -- it selects the LDS slice with scalar arithmetic */
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if ((int)blockIdx.x * W + wave >= n_workers) return; /* the last workgroup of a launch whose worker count is no multiple of W */
    /* The unit of scheduling is a 16x16 luma CELL (8x8 in the chroma planes) -- round 6; until then a 32x32 area, whose four 16x16 blocks ran
     * one after the other behind ONE pair of flags: a 2160p key frame was 187 diagonals of 4 block steps.  Intra prediction of blocks >= 8x8
     * never reads the above-right neighbour, so any order in which a block follows its left, above and above-left neighbours gives the
     * reference's result: cells go in anti-diagonal order (374 diagonals of ONE 16x16 step at 2160p), the blocks inside a cell in z-order.
     * A cell's flag says "this cell and everything it depended on is reconstructed and visible".  A 32x32 block covers 2 x 2 cells: it is
     * coded by the ticket of its TOP-RIGHT cell -- every cell it depends on then lies on an earlier diagonal, so a worker still only ever
     * waits for smaller tickets -- which sets all four flags; the tickets of its other three cells have nothing to do.
     * Which cells are coded, and that every drawn ticket that passes the 32x32 rule publishes its flag, depends on the mode-info grid
     * alone: a malformed unit sets the status bit and its cell still publishes. */
    const int lane = (int)__lane_id(), c_cols = (P.width + 15) >> 4, c_rows = (P.height + 15) >> 4, n_cell = c_cols * c_rows;
    /* a wave on a chain of dependent blocks, beside kernels that fill the SIMDs: it issues rarely, so letting it go first costs
     * the others next to nothing and keeps the chain at the speed it has alone */
    __builtin_amdgcn_s_setprio(3);
  /* workers are persistent: each keeps drawing tickets until they run out -- a launch of one worker per (cell, plane) would keep
     thousands of them resident, nearly all polling flags of cells many diagonals away */
#ifdef INTRA_WALK_PROF
  unsigned long long pf[5] = {0, 0, 0, 0, 0}, pf_n = 0;
  const int worker = (int)blockIdx.x * W + wave;
#endif
  for (;;) {
    /* lane 0 draws; the ticket reaches the wave's other lanes through a scalar register.  The wave meets first: without a convergent
     * operation between the `if (lane == 0)` that closes a round and the one that draws, the compiler threads the two into a path of
     * lane 0's own around the loop, and the lanes no longer arrive at the readfirstlane together */
    tq_block_sync();
    int drawn = 0;
    if (lane == 0) drawn = atomicAdd(&P.sync[0], 1);
    const int ticket = __builtin_amdgcn_readfirstlane(drawn);
#ifdef INTRA_WALK_PROF
    if (ticket >= 3 * n_cell) { if (lane == 0 && worker == 0) printf("[intra-fine] refs %llu predict %llu tq %llu drain %llu (summed over all workers so far)\n", g_intra_fine[0], g_intra_fine[1], g_intra_fine[2], g_intra_fine[3]);
      if (lane == 0 && worker < 2) printf("[intra-prof] worker %d cells %llu: ticket+map %llu wait %llu work %llu drain %llu publish %llu (100 MHz ticks)\n", worker, pf_n, pf[0], pf[1], pf[2], pf[3], pf[4]); break; }
    unsigned long long pt0 = __builtin_amdgcn_s_memtime();
#else
    if (ticket >= 3 * n_cell) break;
#endif
    const int plane = ticket % 3;
    /* the n-th cell in anti-diagonal order (encdec_core.h: the same text runs on the host, where the order is checked for every grid shape) */
    int cr, cc;
    svt_intra_cell_of_ticket(ticket / 3, c_rows, c_cols, &cr, &cc);
    const int cell = cr * c_cols + cc;
    int32_t  *done = P.sync + 2 + plane * n_cell;
    /* what the cell belongs to: the unit at the origin of its 2 x 2 cell group decides (a 32x32 block starts there or nowhere in the group), so
       the four cells of a group agree whatever the grid holds */
    const int  br = cr & ~1, bc = cc & ~1;                                      /* first cell of the group */
    const int  ub_r = br * 2, ub_c = bc * 2;                                     /* its first 8x8 unit */
    const svt_lf_mode_info b0 = P.mi[ub_r * P.mi_stride + ub_c];
    const bool big = b0.sb_type == 9 && !(b0.is_inter && P.mixed) && ub_r + 4 <= P.mi_rows && ub_c + 4 <= P.mi_cols; /* a 32x32 block coded in this pass */
    if (big && !(cr == br && cc == bc + 1)) continue;                            /* its top-right cell's ticket codes it and sets the four flags */
    const int ur0 = cr * 2, uc0 = cc * 2;
#ifdef INTRA_WALK_PROF
    unsigned long long pt1 = __builtin_amdgcn_s_memtime();
#endif
    if (lane == 0) {
        /* (r, c - 1) and (r - 1, c); for the 32x32 block at (br, bc): its lowest left neighbour (br + 1, bc - 1) and its rightmost above
           neighbour (br - 1, bc + 1) -- the flags of the cells before them on their row / column were waited for by THEIR owners */
        const int wl_r = big ? br + 1 : cr, wl_c = (big ? bc : cc) - 1;
        const int wa_r = (big ? br : cr) - 1, wa_c = big ? bc + 1 : cc;
        if (wl_c >= 0) while (__hip_atomic_load(&done[wl_r * c_cols + wl_c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) __builtin_amdgcn_s_sleep(2);
        if (wa_r >= 0) while (__hip_atomic_load(&done[wa_r * c_cols + wa_c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) __builtin_amdgcn_s_sleep(2);
    }
    tq_block_sync(); /* the wave's reference-sample loads stay behind lane 0's flag loads */
#ifdef INTRA_FENCES
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
#ifdef INTRA_WALK_PROF
    unsigned long long pt2 = __builtin_amdgcn_s_memtime();
#endif
    /* the 8x8 units of the cell (of the 32x32 block: only its first unit starts a block) in z-order */
    const int nu = big ? 1 : 4, u_r = big ? ub_r : ur0, u_c = big ? ub_c : uc0;
    for (int z = 0; z < nu; z++) {
        const int r = (z >> 1) & 1, c = z & 1;
        const int ur = u_r + r, uc = u_c + c;
        if (ur >= P.mi_rows || uc >= P.mi_cols) continue;
        const svt_lf_mode_info b = P.mi[ur * P.mi_stride + uc];
        const int sub = b.sb_type == 0; /* an 8x8 unit of four 4x4 luma blocks + one 4x4 chroma block per plane */
        const int w8 = b.sb_type == 3 || sub ? 1 : b.sb_type == 6 ? 2 : b.sb_type == 9 ? 4 : 0;
        if (b.is_inter && P.mixed) continue;
        if (w8 == 0 || b.is_inter) { if (lane == 0) atomicOr(P.status, 1); continue; }
        if ((ur % w8) || (uc % w8)) continue;
        if (w8 == 4 && !big) { if (lane == 0) atomicOr(P.status, 1); continue; } /* a 32x32 block where none can start (or one that leaves the picture): malformed */
        const int mode = plane ? b.pad_[2] : b.pad_[1];
        if (ur + w8 > P.mi_rows || uc + w8 > P.mi_cols || b.tx_size != (sub ? 0 : w8 == 1 ? 1 : w8 == 2 ? 2 : 3) || (!sub && mode > 9) || b.pad_[2] > 9) {
            if (lane == 0) atomicOr(P.status, 1);
            continue;
        }
        const int sb = (ur >> 3) * P.sb_cols + (uc >> 3);
        const int x0 = plane ? uc * 4 : uc * 8, y0 = plane ? ur * 4 : ur * 8, nn = plane ? w8 * 4 : w8 * 8;
        int eob;
        if (sub && plane == 0) { /* blocks 0..3 in the reference's order, each with its own mode (nibbles of pad_[1], pad_[0]) */
            const int m4 = (int)b.pad_[1] | (int)b.pad_[0] << 8;
            eob = 0;
            for (int q4 = 0; q4 < 4; q4++) {
                const int mq = (m4 >> (4 * q4)) & 15;
                if (mq > 9) { if (lane == 0) atomicOr(P.status, 1); continue; }
                eob |= INTRA_WALK_BLOCK(4, 0, x0 + 4 * (q4 & 1), y0 + 4 * (q4 >> 1), mq, sb, !(q4 & 1));
            }
        }
        else if (nn == 32) eob = INTRA_WALK_BLOCK(32, plane, x0, y0, mode, sb, 0);
        else if (nn == 16) eob = INTRA_WALK_BLOCK(16, plane, x0, y0, mode, sb, 0);
        else if (nn == 8) eob = INTRA_WALK_BLOCK(8, plane, x0, y0, mode, sb, 0);
        else eob = INTRA_WALK_BLOCK(4, plane, x0, y0, mode, sb, 0);
        if (eob && lane == 0) P.nz[ur * P.mi_stride + uc] = 1; /* the three planes of a block may all store the same 1 */
    }
#ifdef INTRA_WALK_PROF
    unsigned long long pt3 = __builtin_amdgcn_s_memtime();
#endif
    /* publish the cell (the four cells of a 32x32 block): its reconstruction reaches memory before the flag does */
#ifdef INTRA_FENCES
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    tq_block_sync();
#else
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* every (write-through) store of this wave has completed */
    tq_block_sync(); /* ... and lane 0's flag store stays behind it */
#endif
#ifdef INTRA_WALK_PROF
    unsigned long long pt4 = __builtin_amdgcn_s_memtime();
#endif
    if (lane == 0) {
        if (big) {
            _Pragma("unroll") for (int k = 0; k < 4; k++) {
                const int rr = br + (k >> 1), c2 = bc + (k & 1);
                if (rr < c_rows && c2 < c_cols) __hip_atomic_store(&done[rr * c_cols + c2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else __hip_atomic_store(&done[cell], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#ifdef INTRA_WALK_PROF
    { const unsigned long long pt5 = __builtin_amdgcn_s_memtime(); pf[0] += pt1 - pt0; pf[1] += pt2 - pt1; pf[2] += pt3 - pt2; pf[3] += pt4 - pt3; pf[4] += pt5 - pt4; pf_n++; }
#endif
  }
