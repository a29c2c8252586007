// The body of k_episode_targets and of k_episode_targets_discounted (episode_targets.hip): included once in each, after
// ET_DISCOUNTED is set to 0 or 1.  `A` is the kernel's argument: TargetArgs, or TargetArgsDiscounted with gamma and v_rows.
// (A kernel that calls a shared function instead compiles to other instructions: the included text keeps k_episode_targets'.)
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * ET_WAVES + (threadIdx.x >> 6);
    if (e >= A.n_seg) return;                                   // (wave-uniform: no barrier follows)
    int first = A.seg[e], last = A.seg[e + 1];
    if (first < 0 || last > A.n_rows) {
        if (lane == 0) A.fault[0] = 1;
        first = first < 0 ? 0 : first;
        last = last > A.n_rows ? A.n_rows : last;
    }
    if (first >= last) return;
    const bool tail = A.tail_kind[e] == 1;
    // the carry: what lies behind the chunk in hand (wave-uniform)
    double cN = tail ? (double)A.tail_value[e] : 0.0, cB = tail ? 1.0 : 0.0;
    int cs = tail ? A.tail_score[e] : 0;                        // the score of the next element that exists ...
    bool c_has = tail;                                          // ... if there is one
    int s_end = cs;                                             // mode 0: the tail's score, or the last row's
    bool end_has = tail;
#if ET_DISCOUNTED
    constexpr bool DISC = true;
    const double gamma = A.gamma;
    const float* v_rows = A.v_rows;
#else
    constexpr bool DISC = false;
    constexpr double gamma = 1.0;
    constexpr const float* v_rows = nullptr;
#endif
    const bool discounted_sum = DISC && A.mode == 0 && gamma != 1.0;      // D_i = r_i + gamma D_{i+1} ...
    double cD = 0.0;                                            // ... and its carry

    for (int base = first + ((last - first - 1) / 64) * 64; base >= first; base -= 64) {
        const int j = base + lane;
        const bool in = j < last;
        const int r = in ? A.order[j] : -1;
        const bool ok = in && r >= 0 && r < A.n_rows;
        if (in && !ok) A.fault[0] = 1;
        const uint32_t* row = A.rows + (size_t)(ok ? r : 0) * ET_ROW_DW;
        const int s = ok ? (int)row[ET_SCORE] : 0;
        const uint32_t v_bits = !ok ? 0u : DISC && v_rows != nullptr ? __float_as_uint(v_rows[r]) : row[ET_VALUE];
        const uint32_t var_bits = ok ? row[ET_VARIANCE] : 0u;
        const float v = __uint_as_float(v_bits), var = __uint_as_float(var_bits);

        float out = 0.0f;
        if (A.mode == 2) {
            out = v;
        } else if (A.mode == 0 && !discounted_sum) {
            if (!end_has) {
                const uint64_t have = __ballot(ok);
                if (have) {
                    s_end = __shfl(s, 63 - __builtin_clzll(have));
                    end_has = true;
                }
            }
            out = (float)((long long)s_end - (long long)s);
        } else {
            // the score of the next row that exists, looking past the ones that do not: first inside the chunk ...
            int s_here = s;
            bool has = ok;
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                const int t = __shfl_down(s_here, k);
                const int th = __shfl_down((int)has, k);
                if (!has && lane + k < 64 && th) { s_here = t; has = true; }
            }
            int s_next = __shfl_down(s_here, 1);
            int next_has = __shfl_down((int)has, 1);
            if (lane == 63 || !next_has) { s_next = cs; next_has = c_has; }       // ... then behind it
            const double d = next_has ? (double)((long long)s_next - (long long)s) : 0.0;
            if (discounted_sum) {
                double a = ok ? gamma : 1.0, o = ok ? d : 0.0;                    // D -> o + a D
#pragma unroll
                for (int k = 1; k < 64; k <<= 1) {
                    const double ga = shfl_down_f64(a, k), go = shfl_down_f64(o, k);
                    if (lane + k < 64) { o = o + a * go; a = a * ga; }
                }
                const double D = o + a * cD;
                out = (float)D;
                cD = lane0_f64(D);
            } else {
                Map<DISC> m;
                if (ok) {
                    m.a = DISC ? A.lambda * gamma : A.lambda; m.b = A.lambda * d; m.oN = (double)v; m.oB = 1.0;
                    m.set_aB(A.lambda);
                } else { m.a = 1.0; m.b = 0.0; m.oN = 0.0; m.oB = 0.0; m.set_aB(1.0); }
#pragma unroll
                for (int k = 1; k < 64; k <<= 1) {
                    Map<DISC> g;
                    g.a = shfl_down_f64(m.a, k); g.b = shfl_down_f64(m.b, k);
                    g.oN = shfl_down_f64(m.oN, k); g.oB = shfl_down_f64(m.oB, k);
                    g.set_aB(shfl_down_f64(m.aB(), k));
                    if (lane + k < 64) m = compose(m, g);
                }
                const double N = m.oN + (m.a * cN + m.b * cB), B = m.oB + m.aB() * cB;
                out = (float)(N / B);
                cN = lane0_f64(N);
                cB = lane0_f64(B);
            }
            const int h0 = __shfl((int)has, 0), s0 = __shfl(s_here, 0);
            if (h0) { cs = s0; c_has = true; }
        }

        float w = 1.0f;
        if (A.weight_mode >= 2) {
            const float* st = reinterpret_cast<const float*>(row + ET_VISITS);
            float sum = ok ? st[0] : 0.0f;
#pragma unroll
            for (int a = 1; a < 7; ++a) sum = sum + (ok ? st[a] : 0.0f);
            w = sum;
        }
        if (A.weight_mode == 1 || A.weight_mode == 3) w = w / (var + A.eps);
        if (in) {
            A.value[j] = ok ? out : 0.0f;
            A.variance[j] = __uint_as_float(var_bits);
            A.weight[j] = ok ? w : 0.0f;
        }
    }
