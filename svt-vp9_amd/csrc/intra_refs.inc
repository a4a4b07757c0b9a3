/* intra_refs.inc -- the reference samples of one N x N intra block -> the worker's edge[] in LDS (generate_intra_reference_samples, the
 * paths of a block inside the picture), as text: the one form intra_block (intra_kernel.hip) and intra_rc_block (intra_recon_kernel.hip)
 * both include.  MAY BE INCLUDED ONLY INSIDE A BLOCK BODY, with in scope: N, lane, edge (128 bytes: left column downwards from
 * edge[31], the corner at edge[32], the above row and its right half from edge[33]), rp / rs (the plane's reconstruction and its
 * stride), x0, y0, have_left, have_top, have_right.  The caller's tq_block_sync() follows it. */
    {
        const int j = lane & 31;
        if (lane < 32) { /* left column */
            if (j < N) edge[32 - (j + 1)] = have_left ? INTRA_LD(&rp[(size_t)(y0 + j) * rs + x0 - 1]) : (uint8_t)129;
        } else {         /* above row, replicated to the right */
            if (j < N) {
                const uint8_t a = have_top ? INTRA_LD(&rp[(size_t)(y0 - 1) * rs + x0 + j]) : (uint8_t)127;
                edge[32 + 1 + j] = a;
                /* the right half of the row: true above-right samples for a 4x4 luma block in the left half of its unit (have_right,
                   EbEncDecProcess.c:1146, 1279-1288), copies of the last sample otherwise */
                if (N == 4 && have_right) edge[32 + 1 + N + j] = have_top ? INTRA_LD(&rp[(size_t)(y0 - 1) * rs + x0 + N + j]) : (uint8_t)127;
                else if (j == N - 1) { _Pragma("unroll") for (int q = 0; q < N; q++) edge[32 + 1 + N + q] = a; }
            }
        }
        if (lane == 0) edge[32] = have_top ? (have_left ? INTRA_LD(&rp[(size_t)(y0 - 1) * rs + x0 - 1]) : (uint8_t)129) : (uint8_t)127;
    }
