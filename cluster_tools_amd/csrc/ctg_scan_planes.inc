// The planes of one wave of k_face_scan (ctg_scan.hip), which includes this
// text once per body, inside the kernel, with a constexpr bool INTERIOR in
// scope -- the same statements compiled as straight code for each, so the
// general body is the code it always was.
//
// INTERIOR (face kernels on whole arrays; scan_wave_interior, ctg_plan.h):
// every lane, row and plane of the wave, and the face above each, is owned.
// wave_geometry(true) makes the lane masks, the row masks and the clamps
// constants, so the site masks, the row bit tests, the lane-mask ands and the
// membership terms below fold away -- a push site is the bare ballot of its
// label compare -- and the prefetch never re-reads a plane.  The faces, their
// order, the stage, the capacity tests, the folds, the polls and the flush
// protocol are the same in both bodies.
{
    wave_geometry(INTERIOR);
    if (z0 < z1) {
        load_plane(z0, Ln, Dc, XLn, XDc, Dyc, Dzn, false);
#pragma unroll
        for (int r = 0; r <= ROWS; ++r) Lc[r] = narrow(Ln[r]);
        XLc = narrow(XLn);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): nothing in flight when the plane loop starts
    for (int z = z0; z < z1; ++z) {
        const bool hz = INTERIOR || z + 1 < Z;
        // prefetch of plane z + 1, unconditional (the last plane re-reads
        // itself; its z faces are masked by hz): in flight during the x / y
        // faces, consumed by the z faces (z, z+1) at the end of the plane.
        // (Tried: z faces (z-1, z) against the previous plane, so nothing in
        // a plane waits for the prefetch -- 0.006 ms faster at 512^3, but the
        // changed face order raised records by 23 % at cell 5.)
        if constexpr (RUNNING) next_plane(hz);
        load_plane(hz ? z + 1 : z, Ln, Dn, XLn, XDn, Dyn, Dzn, true);
        const bool zlo = INTERIOR || (z >= obz && z < oez);
        const bool zup = INTERIOR || (hz && z + 1 >= obz && z + 1 < oez);   // face (z, z+1): upper voxel in the own box
        const bool zg = batch && z >= gbz && z < gez;            // graph box planes (batched)
        const bool gzup = zg && z + 1 < gez;
        // this plane's face sites as scalar bit masks (bit r = row r): owned x /
        // y / z faces and (batched) graph-box faces -- tested with scalar bit
        // tests, not carried as per-lane booleans
        const uint32_t s_xo = INTERIOR ? ~0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)(zlo ? row_x : 0u));
        const uint32_t s_yo = INTERIOR ? ~0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)(zlo ? row_y : 0u));
        const uint32_t s_zo = INTERIOR ? ~0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)(zup ? row_x : 0u));
        const uint32_t s_xg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(zg ? grow_x : 0u));
        const uint32_t s_yg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(zg ? grow_y : 0u));
        const uint32_t s_zg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(gzup ? grow_x : 0u));
        if constexpr (MIX) {
            // the channel loop holds most registers: the nearest-neighbour
            // channels of this plane are loaded here, not prefetched with the
            // labels, and die before the loop (x channel rows + x-halo, y
            // channel rows 1..ROWS); the z channel is loaded before the z faces
            const int rmax = Y - 1 - yw;
            const DataT* Ax = D + (int64_t)P.nn_ch[2] * csz + (int64_t)z * sz + (int64_t)yw * X;
            const DataT* Ay = D + (int64_t)P.nn_ch[1] * csz + (int64_t)z * sz + (int64_t)yw * X;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) Dc[r] = load_val_stream<DataT>(Ax, (int64_t)min(r, rmax) * X + xcl);
            XDc = load_val<DataT>(Ax, (int64_t)min(min(lane, ROWS - 1), rmax) * X + xhc);
#pragma unroll
            for (int r = 1; r <= ROWS; ++r) Dyc[r] = load_val_stream<DataT>(Ay, (int64_t)min(r, rmax) * X + xcl);
        }
        if (ablate & 8) {   // diagnostic: loads only
            uint32_t chk = 0;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) chk ^= Lc[r] ^ (uint32_t)Ln[r] ^ __float_as_uint(Dc[r] + Dn[r]);
            if (chk == 0x9E3779B9u && XLc == 7u) atomicAdd(&C->pad[0], 1ull);
        } else {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const uint32_t lc = Lc[r];
                // x face (x, x+1); lane 63 takes its neighbour from the x-halo
                const uint32_t lx = shl1(lc, (uint32_t)__builtin_amdgcn_readlane((int)XLc, r));
                // owned faces carry samples; (batched) sub-graph faces the block
                // does not own go in as adjacency-only entries
                const bool xo = (s_xo >> r) & 1u, xg = BATCH && ((s_xg >> r) & 1u);
                if ((xo || xg) && (!AFF || adj_marks || NNF)) {
                    const float dx = (BND || NNF) ? __uint_as_float(shl1(__float_as_uint(Dc[r]),
                                                                         (uint32_t)__builtin_amdgcn_readlane(
                                                                             (int)__float_as_uint(XDc), r)))
                                                  : 0.f;
                    const bool own = xo && lane_xf;
                    if constexpr (NNF) {   // aff[x channel] of the upper voxel x + 1
                        PUSH(lc != lx, m_xf, own, lc, lx, __float_as_uint(dx), NN_MARK);
                    } else {
                        PUSH(lc != lx, (xo ? m_xf : 0ull) | (xg ? m_gxf : 0ull), own || (xg && glane_xf), lc, lx,
                             (own || !BATCH) ? __float_as_uint(Dc[r]) : MARK_ADJ,
                             (AFF || (BATCH && !own)) ? MARK_ADJ : __float_as_uint(dx));
                    }
                }
                // y face (y, y+1)
                const bool yo = (s_yo >> r) & 1u, yg = BATCH && ((s_yg >> r) & 1u);
                if ((yo || yg) && (!AFF || adj_marks || NNF)) {
                    const bool own = yo && lane_yz;
                    if constexpr (NNF) {   // aff[y channel] of the upper voxel, row r + 1
                        PUSH(lc != Lc[r + 1], m_yz, own, lc, Lc[r + 1], __float_as_uint(Dyc[r + 1]), NN_MARK);
                    } else {
                        PUSH(lc != Lc[r + 1], (yo ? m_yz : 0ull) | (yg ? m_gyz : 0ull), own || (yg && glane_yz), lc,
                             Lc[r + 1],
                             (own || !BATCH) ? __float_as_uint(Dc[r]) : MARK_ADJ,
                             (AFF || (BATCH && !own)) ? MARK_ADJ : __float_as_uint(Dc[r + 1]));
                    }
                }
            }
            // affinity samples aff[c, p] for q = p + o_c, p in the owned box:
            // per channel, the gathers / sample loads of all ROWS rows are in
            // flight together, then their Bloom probes (long-range channels)
            if constexpr (AFF) {
                if (zlo && row_x) {
                    const int64_t iz = (int64_t)z * sz + (int64_t)yw * X + x;
                    const int n_loop = MIX ? P.n_loop : P.n_channels;
                    for (int c0 = 0; c0 < n_loop; c0 += AFF_G) {
                        constexpr int K = AFF_G * ROWS;   // (channel, row) sites of the group
                        uint32_t lq[K];
                        float av[K];
                        bool act[K];
#pragma unroll
                        for (int j = 0; j < AFF_G; ++j) {
                            const bool has = c0 + j < n_loop;
                            const int c = MIX ? (has ? P.loop_ch[c0 + j] : 0) : c0 + j;
                            const int qz = has ? z + P.offsets[c][0] : -1, oy = has ? P.offsets[c][1] : 0;
                            const int qx = has ? x + P.offsets[c][2] : -1;
                            const bool okzx = lane_yz && qz >= 0 && qz < Z && qx >= 0 && qx < X;
#pragma unroll
                            for (int r = 0; r < ROWS; ++r) {
                                const int k = j * ROWS + r;
                                const int qy = yw + r + oy;
                                act[k] = (row_x >> r & 1u) && okzx && qy >= 0 && qy < Y;
                                lq[k] = Lc[r];
                                av[k] = 0.f;
                                if (act[k]) {
                                    // the low half only: every label's high half is
                                    // checked where its own tile loads it
                                    lq[k] = load_lo(L, (int64_t)qz * sz + (int64_t)qy * X + qx);
                                    av[k] = load_val_stream<DataT>(D, (int64_t)c * Z * sz + iz + (int64_t)r * X);
                                }
                            }
                        }
#pragma unroll
                        for (int k = 0; k < K; ++k) act[k] = act[k] && lq[k] != Lc[k % ROWS];
                        // long-range channels: only pairs that are RAG edges
                        // (MIX: every loop channel is long-range)
                        const uint32_t glr = MIX ? (1u << AFF_G) - 1u : (P.lr_mask >> c0) & ((1u << AFF_G) - 1u);
                        if (glr && P.bloom != nullptr && !(ablate & 512)) {
                            uint64_t hb[K];
                            unsigned long long wb[K];
                            uint32_t blk[ROWS];   // the own label's block (owner-blocked filter)
#pragma unroll
                            for (int r = 0; r < ROWS; ++r) blk[r] = bloom_block(Lc[r], P.bloom_mask);
#pragma unroll
                            for (int k = 0; k < K; ++k) {
                                hb[k] = bloom_hash(((uint64_t)Lc[k % ROWS] << 32) | lq[k]);
                                wb[k] = (act[k] && (glr >> (k / ROWS) & 1u)) ? P.bloom[bloom_word(blk[k % ROWS], hb[k])]
                                                                             : ~0ull;
                            }
#pragma unroll
                            for (int k = 0; k < K; ++k)
                                act[k] = act[k] && (wb[k] & bloom_bits(hb[k])) == bloom_bits(hb[k]);
                        }
#pragma unroll
                        for (int j = 0; j < AFF_G; ++j) {
                            if (c0 + j >= n_loop) break;
                            const uint32_t mk = (P.bloom != nullptr && !(glr >> j & 1u)) ? MARK_ONE_ADJ : MARK_ONE;
                            // (nearest-neighbour channels unpaired: A/B nn1024 scan 8.6 -> 9.4 ms paired)
                            if (mk == MARK_ONE && P.bloom != nullptr) {
                                // long-range (or unfiltered) channel: lanes 2i, 2i+1 with the
                                // same key fold as one two-sample entry (along x a cell pair
                                // spans runs of lanes), ~halving this channel's fold work
#pragma unroll
                                for (int r = 0; r < ROWS; ++r) {
                                    const int k = j * ROWS + r;
                                    const uint32_t sv = __float_as_uint(av[k]);
                                    const uint32_t nq = swap1(lq[k]), ns = swap1(sv), nact = swap1(act[k] ? 1u : 0u);
                                    const bool pair = act[k] && nact && nq == lq[k] && ns < MARK_ONE_ADJ &&
                                                      sv < MARK_ONE_ADJ;   // Lc[r] is equal on the pair unless a face
                                    const bool lead = (lane & 1) == 0;
                                    const bool same_c = swap1(Lc[r]) == Lc[r];
                                    const bool pr = pair && same_c;
                                    PUSH(act[k] && !(pr && !lead), ~0ull, true, Lc[r], lq[k], sv,
                                         (pr && lead) ? ns : MARK_ONE);
                                }
                            } else {
#pragma unroll
                                for (int r = 0; r < ROWS; ++r)
                                    PUSH(act[j * ROWS + r], ~0ull, true, Lc[r], lq[j * ROWS + r],
                                         __float_as_uint(av[j * ROWS + r]), mk);
                            }
                        }
                    }
                }
            }
            if constexpr (MIX) {   // the z channel of plane z + 1 (upper voxels of the z faces)
                const int rmax = Y - 1 - yw;
                const DataT* Az = D + (int64_t)P.nn_ch[0] * csz + (int64_t)(hz ? z + 1 : z) * sz + (int64_t)yw * X;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) Dzn[r] = load_val_stream<DataT>(Az, (int64_t)min(r, rmax) * X + xcl);
            }
            // z faces (z, z+1): plane z against the prefetched plane
            if (stamps) {   // diagnostic: how long the prefetched plane keeps this wave waiting
                const uint64_t tw = stamp_now();
                __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
                t_wait += stamp_now() - tw;
            }
            if ((s_zo | s_zg) && (!AFF || adj_marks || NNF)) {
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const bool zo = (s_zo >> r) & 1u, zgr = BATCH && ((s_zg >> r) & 1u);
                    if (zo || zgr) {
                        const bool own = zo && lane_yz;
                        const uint32_t ln = (uint32_t)Ln[r];
                        if constexpr (NNF) {   // aff[z channel] of the upper voxel, plane z + 1
                            PUSH(Lc[r] != ln, m_yz, own, Lc[r], ln, __float_as_uint(Dzn[r]), NN_MARK);
                        } else {
                            PUSH(Lc[r] != ln, (zo ? m_yz : 0ull) | (zgr ? m_gyz : 0ull), own || (zgr && glane_yz),
                                 Lc[r], ln, (own || !BATCH) ? __float_as_uint(Dc[r]) : MARK_ADJ,
                                 (AFF || (BATCH && !own)) ? MARK_ADJ : __float_as_uint(Dn[r]));
                        }
                    }
                }
            }
        }
        // staged entries stay staged across planes (raw faces are valid for
        // whatever table they are folded into later)
        poll();
        // the prefetched plane has landed by now (it had the whole plane's work
        // to do so): wait for it here, before the next plane's loads are
        // issued -- a wait placed after them (where the compiler would put it
        // on first use) would drain the new prefetch too
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
#pragma unroll
        for (int r = 0; r <= ROWS; ++r) {
            Lc[r] = narrow(Ln[r]);
            Dc[r] = Dn[r];
            if constexpr (NN3) {
                if (r >= 1) Dyc[r] = Dyn[r];   // (row 0 of the y channel is never a sample)
            }
        }
        XLc = narrow(XLn);
        XDc = XDn;
    }
}
