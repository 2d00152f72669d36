// ofdm_rx_body.inc — the body of rx_kernel and rx_soft_kernel (ofdm_kernels.hip),
// included as text inside each. In scope there: RxArgs a, SoftArgs sa, the
// template parameters LOGN, STAGED, I16 and the constants SYNC, SOFT.
    using FS = FftShape<LOGN>;
    constexpr int N = FS::N, T = FS::T;
    constexpr int SW = STAGED ? 1 : RX_SMAX;  // register window (symbols)
    extern __shared__ double2 smem[];
    const int S0 = a.S, P0 = a.P;
    double2* bufA = smem;                   // FFT ping-pong images
    double2* bufB = bufA + N;
    double2* lds_tw = bufB + FS::PADN;      // TwLds::SIZE
    double2* pil = lds_tw + TwLds<LOGN>::SIZE;  // S*P raw pilots
    double2* gain = pil + S0 * P0;          // S*P equaliser gains
    double* red = reinterpret_cast<double*>(gain + S0 * P0);
    uint8_t* dec = reinterpret_cast<uint8_t*>(bufA);  // aliases the FFT images after the transforms

    const int t0 = threadIdx.x;
    const int L = N + a.cp;
    const long fstep = gridDim.x;
    // frames to process: a.nframes, or fewer when the count is device-side
    // (speculative stream decode); uniform early exit before any prefetch
    // stream mode: a first frame whose preamble starts before the stream's
    // first sample is the host's (gather path, zeros before sample 0): the
    // frames taken here are fbase, fbase + 1, ...
    const long fbase = (SYNC && a.nframes > 0 && (!a.count || *a.count > 0) && a.starts[0] < 0) ? 1 : 0;
    const long nfr = (a.count ? min(*a.count, a.nframes) : a.nframes) - fbase;
    // Dynamic frames (a.queue): a workgroup's first frame is its blockIdx,
    // later ones come from a counter, so workgroups that run faster (CU and
    // memory-channel placement make them differ by ~15%) take more frames and
    // the kernel ends with the mean workgroup, not the slowest. The last
    // workgroup to leave zeroes the counters for the next launch.
    auto leave = [&]() {
        if (a.queue && threadIdx.x == 0) {
            __threadfence();
            if (atomicAdd(a.queue + 1, 1) == (int)gridDim.x - 1) {
                a.queue[0] = 0;
                a.queue[1] = 0;
            }
        }
    };
    if ((long)blockIdx.x >= nfr) {
        leave();
        return;
    }
    int* qslot = reinterpret_cast<int*>(red + 16);  // the next frame from the queue (red[0..7]: reductions)

    // table loads first, then symbol 0 of the first frame: every prologue wait
    // below is a counted vmcnt that leaves the symbol prefetch in flight
    constexpr bool kTwSplit = T >= TwLds<LOGN>::SIZE;
    TwPiece<LOGN> twp{};
    if constexpr (kTwSplit)
        twp = tw_fetch<LOGN>(a.tab.tw, t0);
    else
        load_twiddles<LOGN>(a.tab.tw, lds_tw, t0, T);
    // data carrier d = t0 + T*i: swizzled LDS slot of its FFT bin (low 16 bits)
    // | pilot slot (high 16); host tables are zero-padded, so no guards here
    int pk[RX_DPT];
#pragma unroll
    for (int i = 0; i < RX_DPT; ++i) pk[i] = a.tab.rx_pack[t0 + T * i];
    const int pbin = a.tab.pilot_swz[t0];
    long fl = blockIdx.x;  // this workgroup's frame
    auto frame_of = [&](long l) { return l + fbase; };
    SymbolRegs<LOGN, I16> pf;
    // sample offset of frame g's first message body (CP strip, Frame.hpp:278-279)
    auto body0 = [&](long g) { return SYNC ? a.starts[g] + a.start_off : g * a.frame_stride + a.cp; };
    dma_symbol<LOGN, I16>(a, body0(frame_of(fl)), bufB, t0);  // grid <= nframes
    if constexpr (kTwSplit) tw_store<LOGN>(twp, lds_tw);
    lds_barrier();  // twiddle table visible: fft_pp reads a pass's twiddles before its barrier

    unsigned long long errs = 0;

    // Persistent over frames (grid <= 2 workgroups per CU): the next frame's
    // symbol 0 is fetched (LDS-DMA into bufB) while this frame's epilogue
    // runs, so HBM reads do not stop between frames, and the tables are
    // loaded once per workgroup.
#pragma unroll 1
    for (long fnext; fl < nfr; fl = fnext) {
        const long f = frame_of(fl);
        OFDM_PHASE(rx_symbols);
        // Opaque per-frame copies of the thread index, the carrier tables and
        // the geometry: everything derived from them is recomputed per frame
        // instead of being hoisted out of the frame loop and held live beside
        // the register window (which spills).
        int t;
        asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"(t0));
#pragma unroll
        for (int i = 0; i < RX_DPT; ++i) asm volatile("" : "+v"(pk[i]));
        int S = a.S, D = a.D, P = a.P;
        asm volatile("" : "+s"(S), "+s"(D), "+s"(P));
        const long x0 = body0(f);
        const int m = 1 << (a.k / 2);
        const double s1 = a.k == 1 ? 0.0 : 1.0 / (2.0 / (m - 1));
        const bool whole_frame_dec = (long)S * D <= (long)FS::PADN * 16;
        const long bpf = a.bytes_per_frame;
        // word-wise packing: k in {1,2,4,8}, whole words, 4-byte aligned outputs
        const bool by_word = (a.k == 1 || a.k == 2 || a.k == 4 || a.k == 8) && (bpf & 3) == 0 &&
                             ((uintptr_t)a.bytes & 3) == 0 && ((uintptr_t)a.ref & 3) == 0;
        // SOFT: this frame's scale (one uniform load), the demapper's
        // constants and the frame's first LLR; a point's k LLRs go out as one
        // group where the output is 16-byte aligned
        SoftScale sq{};
        char* llr_f = nullptr;
        int llr_esz = 0;
        bool llr_vec = false;
        if constexpr (SOFT) {
            sq = soft_scale(a.k, sa.frame_scale ? sa.scale * sa.frame_scale[f] : sa.scale);
            llr_esz = sa.fmt == LLR_F32 ? 4 : 1;
            llr_f = static_cast<char*>(sa.llr) + f * S * D * a.k * llr_esz;
            llr_vec = ((uintptr_t)sa.llr & 15) == 0;
        }
        double2 y[SW][RX_DPT];
        // symbol 0 is read from bufB, so pass 0 writes bufA (free: the
        // previous epilogue ended with a barrier)
        double2* first = bufA;
        double2* second = bufB;
        // One symbol step. With the register window (!STAGED) the steps are
        // straight-line code, s and the window row W compile-time: the put's
        // LDS reads land in the window's own registers, and the allocator
        // has no rolled loop to split the window's live range around (it
        // copied half the window per symbol in each direction). STAGED keeps
        // one rolled step (W = 0 names no register there).
        auto step = [&](int s, auto wc) __attribute__((always_inline)) {
            constexpr int W = decltype(wc)::value;
            double2 v[8];
            if (s == 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of symbol 0 landed
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = stage_get<LOGN, I16>(bufB, t + T * i);
                // the reads stay in this branch: in the rolled step they were
                // merged with pf.get's below into loads through a select of
                // the two pointers, which kept pf in scratch memory
                asm volatile("" ::: "memory");
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = pf.get(i);
            }
            if constexpr (SYNC) {
                // sample m = t + T*i of the body: *= e^{i(A + B m)}, by a
                // running product from e^{i(A + B t)} in steps of e^{i B T};
                // e^{i(A + B t)} from the table (uniform loads), the bits of t
                // selecting its powers (x (1, 0) is exact)
                // (the bit tests on a per-symbol opaque copy of t: hoisted
                // out of the loop, their lane masks filled the SGPRs and spilled)
                const double2* rt = a.corr + (f * S + s) * CORR_PER_SYM;
                int tr;
                asm volatile("v_mov_b32 %0, %1" : "=v"(tr) : "v"(t));
                double2 c = rt[0];
#pragma unroll
                for (int j = 0; j < LOGN - 3; ++j) c = cmul_exact(c, (tr >> j) & 1 ? rt[1 + j] : make_double2(1.0, 0.0));
                const double2 w = rt[CORR_PER_SYM - 1];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    v[i] = cmul(v[i], c);
                    if (i < 7) c = cmul(c, w);
                }
            }
            // opaque copy of t: the per-pass LDS addresses are recomputed each
            // symbol instead of being hoisted out of the loop and held live
            // beside the register window
            int tl;
            asm volatile("v_mov_b32 %0, %1" : "=v"(tl) : "v"(t));
            // fft_pp in two parts, the next symbol's prefetch issued between
            // them: pass 0 reads the prefetch registers themselves (no copy
            // into the transform's registers), and they are free to be
            // reloaded once it has written to LDS. SYNC: the phase ramp's
            // sincos temporaries are dead by then as well (live beside the 8
            // prefetch registers, they spilled at N = 512).
            stockham_pass<LOGN, 8, 1, -1>(v, tl, lds_tw, first);
            asm volatile("" ::: "memory");  // keep the prefetch below pass 0
            if (s + 1 < S) pf.load(a, x0 + (long)(s + 1) * L, t);
            fft_pp_tail<LOGN, 1, -1>(v, tl, lds_tw, second, first, NoHook());
            double2* res = (FftPasses<LOGN>::value & 1) ? first : second;
            first = res == bufA ? bufB : bufA;
            second = res;
            if (t < P) pil[s * P + t] = res[pbin];
            if constexpr (STAGED) {
#pragma unroll
                for (int i = 0; i < RX_DPT; ++i) {
                    const int d = t + T * i;
                    if (d < D) a.ystage[(f * S + s) * D + d] = res[pk[i] & 0xffff];
                }
            } else {
#pragma unroll
                for (int i = 0; i < RX_DPT; ++i) y[W][i] = res[pk[i] & 0xffff];
            }
        };
        if constexpr (STAGED) {
#pragma unroll 1
            for (int s = 0; s < S; ++s) step(s, std::integral_constant<int, 0>{});
        } else {
            do {  // steps 0 .. RX_SMAX-1, left at the first s >= S (uniform)
#define OFDM_RX_STEP(W) \
    if (W >= S) break;  \
    step(W, std::integral_constant<int, W>{});
                OFDM_RX_STEP(0) OFDM_RX_STEP(1) OFDM_RX_STEP(2) OFDM_RX_STEP(3)
                OFDM_RX_STEP(4) OFDM_RX_STEP(5) OFDM_RX_STEP(6) OFDM_RX_STEP(7)
#undef OFDM_RX_STEP
            } while (false);
            static_assert(RX_SMAX == 8, "one OFDM_RX_STEP per window row");
        }
        lds_barrier();  // pilots of the last symbol visible; every thread is done reading bufB
        OFDM_PHASE(rx_phys_gains);
        // The channel carriers go to LDS (bufA past the decisions) by DMA
        // issued ahead of the next frame's symbol 0: read per point from HBM
        // behind that DMA (in-order returns), they cost the stream rx ~18%.
        const double2* chan = a.chan ? a.chan + f * a.chan_stride : nullptr;
        const int dec_b = (S * D + 15) & ~15;
        double2* chl = reinterpret_cast<double2*>(reinterpret_cast<char*>(bufA) + dec_b);
        const bool chan_lds = chan && dec_b + D * 16 <= N * 16;  // uniform
        if (chan_lds) dma_chan<LOGN>(chan, D, chl, t);
        // The emit's fast path (below): hard decisions of k = 2 without a
        // channel, every 64-carrier group of a wave (d = w0 + T*g + lane)
        // wholly inside or outside D, word-aligned outputs. Uniform.
        // (emit_fast and its helpers are written for k = 4 as well; at 16-QAM
        // they measured no gain over the LDS path, DESIGN section 4, so k = 4
        // stays there and the kernel instantiates K = 2 only.)
        bool fast = false;
        if constexpr (!SOFT && !STAGED && !SYNC && T >= 64)
            fast = a.dec_fast && !chan && a.k == 2 && (D & 63) == 0 && by_word &&
                   ((uintptr_t)a.ref & 15) == 0;
        // Its reference bytes go to LDS (bufA: free since the pilot barrier,
        // and this path keeps no decisions there) by the channel's DMA, ahead
        // of the emit's first store and behind the gains: vmcnt counts stores
        // too, so a load issued after the frame's stores would wait for all
        // of them. bpf is a multiple of 16 here and bpf / 16 <= T.
        uint8_t* refl = reinterpret_cast<uint8_t*>(bufA);
        const bool ref_lds = fast && a.ref;  // uniform
        if (ref_lds)
            dma_chan<LOGN>(reinterpret_cast<const double2*>(a.ref + f * bpf), (int)(bpf >> 4),
                           reinterpret_cast<double2*>(refl), t);
        // Static frame order (no queue; the stream decode): the next frame's
        // symbol 0 streams into bufB (free since the pilot barrier) from here,
        // behind the channel carriers, so it overlaps the gains as well.
        // With the queue the next frame is asked for now, its answer awaited
        // after the gains (the register holding it is live across the gains
        // only), and its DMA issued after them.
        const bool early = !a.queue;  // uniform
        if (early) {
            fnext = fl + fstep;
            if (fnext < nfr) dma_symbol<LOGN, I16>(a, body0(frame_of(fnext)), bufB, t);
        }
        int qv = 0;
        if (a.queue && t == 0) qv = atomicAdd(a.queue, 1);

        // phys_pilot_ampl = sum |pilot| / (P*S*pilot_ampl)   (Frame.cpp:76-80)
        double acc = 0.0;
        for (int i = t; i < S * P; i += T) acc += hypot(pil[i].x, pil[i].y);
        acc = block_sum_lds<T>(acc, red);
        const double phys = acc / ((double)(P * S) * a.pilot_ampl);

        // out = (F/phys) / ((F[s,p]/phys) / (F[0,p]/phys)) = F * gain[s][j]   (Frame.cpp:82-93)
        for (int i = t; i < S * P; i += T) {
            const int j = i % P;
            const double2 c0 = make_double2(pil[j].x / phys, pil[j].y / phys);
            const double2 cs = make_double2(pil[i].x / phys, pil[i].y / phys);
            const double2 coef = cdiv_exact(cs, c0);
            const double2 g = cdiv_exact(make_double2(1.0, 0.0), coef);
            gain[i] = make_double2(g.x / phys, g.y / phys);
        }
        if (chan_lds || ref_lds) {  // that DMA landed (the 8 symbol-0 transfers issued after it may still fly)
            if (early && fnext < nfr)
                asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (a.queue && t == 0) *qslot = qv;
        lds_barrier();
        if (!early) {
            // symbol 0 of the next frame streams into bufB behind the emit and
            // the packing
            fnext = fstep + __builtin_amdgcn_readfirstlane(*qslot);  // uniform: an SGPR
            if (fnext < nfr) dma_symbol<LOGN, I16>(a, body0(frame_of(fnext)), bufB, t);
        }

        // One symbol's RX_DPT points of the register window. Without a
        // channel (the common case) the group's gain loads are issued first
        // and the points then computed, stored and decided; the uniform
        // branches are taken once per group, so the points' LDS latencies
        // overlap. With a channel, one point at a time (register pressure).
        auto emit_point = [&](int s, int i, double2 yv) {
            // opaque: the per-point addresses are computed here, not hoisted
            // out of the emit loop and held (32 of them) across it
            int d = t + T * i, gi = s * P + (pk[i] >> 16);
            asm volatile("" : "+v"(d), "+v"(gi));
            double2 o = cmul_exact(yv, gain[gi]);
            if (a.read_out) store_nt(a.read_out + (f * S + s) * D + d, o);
            const double2 cv = chan_lds ? chl[d] : load_untracked(chan + d);
            o = a.chan_recip ? cmul_exact(o, cv) : cdiv_exact(o, cv);
            if (a.constell) store_nt(a.constell + (f * S + s) * D + d, o);
            if constexpr (SOFT)
                soft_emit(o, a.k, s1, sq, sa.fmt, llr_f + (long)(s * D + d) * (a.k * llr_esz), llr_vec);
            dec[whole_frame_dec ? s * D + d : d] = (uint8_t)decide(o, a.k, s1, m);
        };
        // Without a channel (the common case) a group is straight-line code:
        // the output branch is taken once per group and the decision is
        // branch-free, so the scheduler can overlap the points' LDS reads.
        auto emit_plain = [&](int s, const double2 (&yw)[RX_DPT], auto with_store) {
            double2* cbase = a.constell + (f * S + s) * D;
#pragma unroll
            for (int i = 0; i < RX_DPT; ++i) {
                int d = t + T * i, gi = s * P + (pk[i] >> 16);
                asm volatile("" : "+v"(d), "+v"(gi));  // opaque: not hoisted and held
                if (d < D) {
                    const double2 o = cmul_exact(yw[i], gain[gi]);
                    if constexpr (decltype(with_store)::value) store_nt(cbase + d, o);
                    if constexpr (SOFT)
                        soft_emit(o, a.k, s1, sq, sa.fmt, llr_f + (long)(s * D + d) * (a.k * llr_esz), llr_vec);
                    dec[whole_frame_dec ? s * D + d : d] = (uint8_t)decide_select(o, a.k, s1, m);
                }
            }
        };
        auto emit_group = [&](int s, const double2 (&yw)[RX_DPT]) {
            if (SYNC || chan) {  // the stream decode always has its channel
#pragma unroll
                for (int i = 0; i < RX_DPT; ++i)
                    if (t + T * i < D) emit_point(s, i, yw[i]);
            } else if (a.constell) {
                emit_plain(s, yw, std::true_type{});
            } else {
                emit_plain(s, yw, std::false_type{});
            }
        };

        // The fast path's symbol: the unchanged cmul_exact and constellation
        // store per point, the decision as threshold compares (decide_tau),
        // and the symbol's output words assembled in the wave (emit_words):
        // no decision goes through LDS and no packing pass follows. The
        // active groups (g < na, uniform) are straight-line code and their
        // gain reads are issued together; the collecting lanes store the
        // words and count the bit errors against the reference in LDS.
        auto emit_fast = [&](int s, const double2 (&yw)[RX_DPT], auto kc) {
            constexpr int K = decltype(kc)::value, LPB = 8 / K;
            const double tau[DEC_TAU_MAX] = {a.dec_tau[0], a.dec_tau[1], a.dec_tau[2]};
            // opaque copy of the thread index: everything derived from it is
            // computed per symbol, not hoisted out of the emit loop and held
            // (eight symbols' worth) beside the register window
            int tt;
            asm volatile("v_mov_b32 %0, %1" : "=v"(tt) : "v"(t));
            const int lane = tt & 63;
            const int w0 = __builtin_amdgcn_readfirstlane(tt & ~63);
            const int na = w0 < D ? min((D - w0 + T - 1) / T, RX_DPT) : 0;  // uniform: this wave's groups inside D
            double2* cbase = a.constell + (f * S + s) * D;
            double2 gv[RX_DPT];
#pragma unroll
            for (int i = 0; i < RX_DPT; ++i) {
                int gi = s * P + (pk[i] >> 16);
                asm volatile("" : "+v"(gi));
                gv[i] = gain[gi];
            }
            unsigned bits = 0;
#pragma unroll
            for (int i = 0; i < RX_DPT; ++i) {
                const double2 o = cmul_exact(yw[i], gv[i]);
                int d = tt + T * i;
                asm volatile("" : "+v"(d));
                if (a.constell && i < na) store_nt(cbase + d, o);
                bits |= decide_tau<K>(o, tau) << (8 * i);
            }
            unsigned w[K / 2];
            emit_words<K>(bits, lane, w);
            if (emit_collects<K>(lane)) {
#pragma unroll
                for (int h = 0; h < K / 2; ++h) {
                    const int g = (lane & (LPB - 1)) + LPB * h;
                    if (g < na) {
                        // byte offset of this lane's word within the frame
                        const int off = (((s * D + w0 + T * g) * K) >> 3) + 4 * (lane / (4 * LPB));
                        if (a.bytes) *reinterpret_cast<uint32_t*>(a.bytes + f * bpf + off) = w[h];
                        if (a.ref) errs += __popc(w[h] ^ *reinterpret_cast<const uint32_t*>(refl + off));
                    }
                }
            }
        };

        auto pack = [&](long jb0, long jb1, long dbase) {
            for (long jb = jb0 + t; jb < jb1; jb += T) {
                int byte = 0;
                if (a.k == 1 || a.k == 2 || a.k == 4 || a.k == 8) {
                    const int per = 8 / a.k;
                    const long p0 = (jb - jb0) * per + dbase;
                    for (int r = 0; r < per; ++r) byte = (byte << a.k) | dec[p0 + r];
                } else {
                    for (int b = 0; b < 8; ++b) {
                        const long bit = (jb - jb0) * 8 + b;
                        const long g = bit / a.k + dbase;
                        const int within = (int)(bit % a.k);
                        byte = (byte << 1) | ((dec[g] >> (a.k - 1 - within)) & 1);
                    }
                }
                if (a.bytes) a.bytes[f * bpf + jb] = (uint8_t)byte;
                if (a.ref) errs += __popc((unsigned)(byte ^ a.ref[f * bpf + jb]));
            }
        };

        auto pack_words = [&]() {
            const int per_word = 32 / a.k;  // decisions per output word
            for (long w = t; w < bpf / 4; w += T) {
                const uint8_t* dw = dec + w * per_word;
                uint32_t word;
                switch (a.k) {
                    case 1: word = pack_word<1>(dw); break;
                    case 2: word = pack_word<2>(dw); break;
                    case 4: word = pack_word<4>(dw); break;
                    default: word = pack_word<8>(dw); break;
                }
                if (a.bytes) reinterpret_cast<uint32_t*>(a.bytes + f * bpf)[w] = word;
                if (a.ref) errs += __popc(word ^ reinterpret_cast<const uint32_t*>(a.ref + f * bpf)[w]);
            }
        };

        if (fast) {  // only ever true where the constexpr below holds
            if constexpr (!SOFT && !STAGED && !SYNC && T >= 64) {
                OFDM_PHASE(rx_emit_fast);
#pragma unroll 1
                for (int w = 0; w < S; ++w) {
                    switch (w) {
#define OFDM_RX_FAST(W)                                           \
    case W:                                                       \
        if constexpr (W < SW) {                                   \
            emit_fast(w, y[W], std::integral_constant<int, 2>{}); \
        }                                                         \
        break;
                        OFDM_RX_FAST(0) OFDM_RX_FAST(1) OFDM_RX_FAST(2) OFDM_RX_FAST(3)
                        OFDM_RX_FAST(4) OFDM_RX_FAST(5) OFDM_RX_FAST(6) OFDM_RX_FAST(7)
#undef OFDM_RX_FAST
                        default: break;
                    }
                }
                // No barrier and no packing pass here: the decisions never
                // went to LDS (`dec`, the alias of the FFT image, is not
                // written on this path), so the barrier that ordered the dec
                // writes before pack_words' reads has nothing to order. pil,
                // gain, red and the queue slot are still ordered by the
                // frame's last barrier below.
            }
        } else if constexpr (!STAGED) {
            OFDM_PHASE(rx_emit);
            // one symbol per (non-unrolled) iteration: a case's register
            // indices are compile-time, and the scheduler cannot interleave
            // symbols (the next frame's symbol 0 is live in registers here)
#pragma unroll 1
            for (int w = 0; w < S; ++w) {
                if constexpr (SOFT) {
                    // the demapper makes a group several times longer: the
                    // symbol's points are copied out of the window first, so
                    // the group is compiled once, not once per case
                    double2 yw[RX_DPT] = {};
                    switch (w) {
#define OFDM_RX_TAKE(W)                                                        \
    case W:                                                                    \
        if constexpr (W < SW) {                                                \
            _Pragma("unroll") for (int i = 0; i < RX_DPT; ++i) yw[i] = y[W][i]; \
        }                                                                      \
        break;
                        OFDM_RX_TAKE(0) OFDM_RX_TAKE(1) OFDM_RX_TAKE(2) OFDM_RX_TAKE(3)
                        OFDM_RX_TAKE(4) OFDM_RX_TAKE(5) OFDM_RX_TAKE(6) OFDM_RX_TAKE(7)
#undef OFDM_RX_TAKE
                        default: break;
                    }
                    emit_group(w, yw);
                    continue;
                }
                switch (w) {
#define OFDM_RX_EMIT(W)                 \
    case W:                             \
        if constexpr (W < SW) {         \
            emit_group(w, y[W]);        \
        }                               \
        break;
                    OFDM_RX_EMIT(0) OFDM_RX_EMIT(1) OFDM_RX_EMIT(2) OFDM_RX_EMIT(3)
                    OFDM_RX_EMIT(4) OFDM_RX_EMIT(5) OFDM_RX_EMIT(6) OFDM_RX_EMIT(7)
#undef OFDM_RX_EMIT
                    default: break;
                }
            }
            lds_barrier();
            OFDM_PHASE(rx_pack);
            if (by_word)
                pack_words();
            else
                pack(0, bpf, 0);
        } else {
            OFDM_PHASE(rx_emit);
            const long bps = (long)D * a.k / 8;  // bytes per symbol (host checks D*k % 8 == 0)
            for (int s = 0; s < S; ++s) {
                double2 yst[RX_DPT];
#pragma unroll
                for (int i = 0; i < RX_DPT; ++i)
                    yst[i] = t + T * i < D ? a.ystage[(f * S + s) * D + t + T * i] : make_double2(0.0, 0.0);
                emit_group(s, yst);
                lds_barrier();
                if (!whole_frame_dec) {
                    pack(s * bps, (s + 1) * bps, 0);
                    lds_barrier();
                }
            }
            if (whole_frame_dec) pack(0, bpf, 0);
        }
        OFDM_PHASE(rx_frame_end);
        lds_barrier();  // dec (or the fast path's reference bytes) / pil / gain / red are rewritten by the next frame
    }
    OFDM_PHASE(rx_end);
    if (a.bit_errors) {
        errs = block_sum_u64<T>(errs, red);
        if (t0 == 0 && errs) atomicAdd(a.bit_errors, errs);
    }
    leave();
