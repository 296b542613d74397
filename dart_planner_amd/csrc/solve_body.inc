// solve_body.inc -- ONE solve by the G lanes of a group: everything between "the problem's data are in registers" and "the solution is in
// registers" -- cold start (or the caller's x0), projection, the L-BFGS-B iterations.  Textually included (not a function: handing the
// parameter block and the nine variables through a call boundary cost the packed kernels 70 spilled registers) by solve_kernel (one
// solve per group and launch, solve_kernel.hip) and by the closed-loop Monte-Carlo kernel (one solve per group and planning cycle,
// monte_carlo.hip).  The including scope provides:
//   template parameters IO, G;  constexpr int P = kWave / G, J = kSlots;  const SolveDev q;  unsigned char* lds_raw;
//   const int lane, k (= lane & (G - 1)), grp (= lane / G);  const double ps[3], vs[3], goal[3] (identical in the group's lanes);
//   const IO* x0row (NULL = the reference's cold start, else this problem's [9N] start);  const bool cold = x0row == nullptr;
//   double x[J] (the lane's nine variables P_k, V_k, T_k on exit);  SE3MPC_TICK's tsec / tlast under SE3MPC_SOLVE_PROFILE;
// and finds afterwards: double f; int nit, nfev, status, task (and everything else the body declares, in the including block's scope).
  const int n = q.n, N = q.N, n3 = 3 * q.N;
  // Two-tier memory: the first launch gives every problem LDS for `mlds` L-BFGS pairs (2-4: all a solve with the reference's options
  // ever stores -- it stops after 1-3 iterations, i.e. at most two updates) so that two wavefronts per SIMD fit a CU's LDS; a
  // problem that needs a pair more leaves with task = SE3MPC_TASK_OVERFLOW and is re-solved from scratch by the second launch
  // (mlds = maxcor, only_overflow = 1), in which every other group exits at once.  `m` below is the STORAGE bound; the
  // algorithm's memory is still q.m.
  const int m = q.mlds;
  // LDS carve-up: per-problem small matrices (doubles) first, then the S / Y pairs of the whole wavefront in the IO type
  double* sy = reinterpret_cast<double*>(lds_raw) + grp * small_doubles(m);   // [m][m]  S'Y (lower triangle used)
  double* ss = sy + m * m;                             // [m][m]  S'S (upper triangle used)
  double* wt = ss + m * m;                             // [m][m]  Cholesky factor of theta*S'S + L D^-1 L'
  double* wn = wt + m * m;                             // [2m][2m] LEL' factor of the subspace K matrix
  double* pv = wn + 4 * m * m;                         // [2m]  p = W'd            (Cauchy)
  double* cv = pv + 2 * m;                             // [2m]  c = W'(xcp - x)    (Cauchy)
  double* vv = cv + 2 * m;                             // [2m]  scratch M*...
  double* wbp = vv + 2 * m;                            // [2m]  row of W at a breakpoint
  double* wv = wbp + 2 * m;                            // [2m]  subspace rhs
  double* sc = wv + 2 * m;                             // [8]   scalars handed out of scalar sections
  // pairs: [m][64 lanes][LS] -- a lane's row of one pair holds its nine (s_j, y_j) couples contiguously (18 values + padding to a
  // multiple of 16 bytes whose dword stride, 20 for float / 36 for double, keeps 16-byte reads of the 16 lanes of a group in
  // disjoint banks): one pass over a pair is five (float) or nine (double) ds_read_b128 per lane instead of eighteen ds_read_b32,
  // each of which the register-starved schedule waited for on its own (SQ_WAIT_ANY was 45 % of a lone wavefront's cycles).
  constexpr int LS = pair_row_values<IO>();
  IO* pairs = reinterpret_cast<IO*>(lds_raw + pairs_offset_bytes(P, m));

  // ---- per-lane facts and problem data
  const bool live = k < N;                 // k >= N: padding lane, its nine variables are fixed at 0
  const bool last = k == N - 1;            // terminal position row
  // the goal coordinate the objective sees: 0 on a padding lane, whose position slots then have gradient 0 like its other slots
  double gl[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) gl[a] = live ? goal[a] : 0.0;

  // ---- cold start (planner.py:329-359) or caller x0, projected into the box (L-BFGS-B `active`)
  double g[J], z[J], d[J], xo[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int blk = j / 3, a = j % 3;
    double xv = 0.0;
    if (!cold) {
      xv = live ? (double)x0row[blk * n3 + 3 * k + a] : 0.0;
    } else {
      const double denom = (double)(N - 1 > 1 ? N - 1 : 1);
      if (blk == 0) {
        const double alpha = (double)k / denom;
        xv = q.has_goal ? (1.0 - alpha) * ps[a] + alpha * goal[a] : ps[a];
      } else if (blk == 1) {
        if (q.has_goal) {
          const double a1 = (double)k / denom, a0 = (double)(k - 1) / denom;
          xv = (((1.0 - a1) * ps[a] + a1 * goal[a]) - ((1.0 - a0) * ps[a] + a0 * goal[a])) / q.dt;
        }
        xv = (k == 0) ? vs[a] : xv;
      } else {
        xv = (a == 2) ? q.hover : 0.0;
      }
    }
    x[j] = live ? fmin(fmax(xv, box_lo(q, j)), box_hi(q, j)) : 0.0;
    g[j] = 0.0; z[j] = x[j]; d[j] = 0.0; xo[j] = x[j];
  }

  // the reference's gradient (planner.py:552-580) of one slot.  The same expression wherever a gradient value is needed again (the
  // previous iterate's gradient in the BFGS update and after a failed line search is RECOMPUTED from the saved x, not kept in nine more
  // register pairs); contraction off so that both places round the product the same way.
  auto grad_of = [&](int j, double xv) -> double {
#pragma clang fp contract(off)
    if (j < 3) return q.has_goal ? q.two_wp * (xv - gl[j]) : 0.0;
    if (j < 6) return q.two_wv * xv;
    return q.two_wT * xv;
  };
  // objective (planner.py:516-550) and gradient at x; with_gd: also g(x)'d, its reduction interleaved with the objective's (the
  // line search wants both)
  // A line-search evaluation (with_gd) does not store the gradient: it only needs g(x)'d, and the nine gradient values are formed again
  // from x when the search has ended -- so that no gradient registers are live across the line search, the kernel's pressure peak.
  double gd_fused = 0.0;
  auto eval_fg = [&](bool with_gd = false) -> double {
    double part = 0.0, gdp = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (q.has_goal) {
        const double e = x[a] - gl[a];
        double fj = q.wp * (e * e);
        const double ft = q.term_wp * (e * e);
        fj = last ? fj + ft : fj;
        part += fj;
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double xv = x[3 + a];
      part += q.wv * (xv * xv);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double xv = x[6 + a];
      const double ac = xv / q.mass - (a == 2 ? q.grav : 0.0);
      const double dv = xv - (a == 2 ? q.hover : 0.0);
      part += q.wa * (ac * ac) + q.wT * (dv * dv);
    }
    part = live ? part : 0.0;
    if (with_gd) {
#pragma unroll
      for (int j = 0; j < J; ++j) gdp += grad_of(j, x[j]) * (z[j] - xo[j]);      // d = z - x_old, formed here (see opaque())
      double r2[2] = {part, gdp};
      group_sum_n<G, 2>(r2);
      gd_fused = r2[1];
      return r2[0];
    }
#pragma unroll
    for (int j = 0; j < J; ++j) g[j] = grad_of(j, x[j]);
    return group_sum<G>(part);
  };
  // projected gradient norm (projgr)
  auto projgr = [&]() -> double {
    double mx = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const double gj = g[j];
      const double up = fmax(x[j] - box_hi(q, j), gj), dn = fmin(x[j] - box_lo(q, j), gj);      // both sides, then one select: no divergent branches
      const double gi = gj < 0.0 ? up : dn;
      mx = fmax(mx, fabs(gi));
    }
    mx = live ? mx : 0.0;
    return group_max<G>(mx);
  };
  auto ROW = [&](int c) -> IO* { return static_cast<IO*>(__builtin_assume_aligned(pairs + (c * kWave + lane) * LS, 16)); };
  auto WS = [&](int c, int j) -> IO& { return ROW(c)[2 * j]; };
  auto WY = [&](int c, int j) -> IO& { return ROW(c)[2 * j + 1]; };

  // ---- L-BFGS-B state (identical in every lane of the group)
  int col = 0, iupdat = 0, iter = 0, nit = 0;
  double theta = 1.0;
  int iwhere[J];
#pragma unroll
  for (int j = 0; j < J; ++j) iwhere[j] = live ? 0 : 3;   // padding = fixed variables
  // nfev counts like scipy's ScalarFunction: asking again for the x evaluated last (a line search whose steps shrank below
  // rounding) returns the same (f, g) and is not counted.  x_is_last: the registers x hold the x of the last evaluation.
  int nfev = 1;
  bool x_is_last = true;
  double f = eval_fg();
  double sbgnrm = projgr();
  int status = 0, task = 0;
  double fold = f;

  if (sbgnrm <= q.pgtol) { task = SE3MPC_TASK_CONV_PGTOL; status = 0; }

  SE3MPC_TICK(0)
  int guard = 0;                           // every pass either ends an iteration or drops the memory; bounded anyway
  while (task == 0) {
    if (++guard > 4 * (q.maxiter + 8)) { task = SE3MPC_TASK_ABNORMAL; status = 2; break; }
    // ===================================================================== Cauchy point
    int info = 0;
    {
      // pass 1: search direction d = -g on the free variables, breakpoints, p = W'd, f1 = -d'd
      double tbp[J];
      double f1p = 0.0;
      int nbr = 0;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        // written as value selects throughout: as nested ifs this loop became ~50 exec-mask instructions per slot
        const double lo = box_lo(q, j), hi = box_hi(q, j);
        const double neggi = -g[j];
        const double tl = x[j] - lo, tu = hi - x[j];
        const bool xlower = tl <= 0.0, xupper = tu <= 0.0;
        const int atlo = neggi <= 0.0 ? 1 : 0, athi = neggi >= 0.0 ? 2 : 0, flat = fabs(neggi) <= 0.0 ? -3 : 0;
        const int iwb = xlower ? atlo : (xupper ? athi : flat);
        const int iw = live ? iwb : 3;                       // (nothing of the previous iterate's iwhere survives but "padding lane" = fixed)
        iwhere[j] = iw;
        const bool moving = iw == 0;
        const double dj = moving ? neggi : 0.0;
        d[j] = dj;
        f1p -= dj * dj;
        // breakpoint t_j = num / |g_j| (tl / (-neggi) for a descending, tu / neggi for an ascending variable).  Only the numerator is kept here:
        // the quotient is formed where a breakpoint's VALUE is needed -- never on the first iterate (theta = 1: t_j <= 1 <=> num <= |g_j|, exactly)
        // and not on an iterate whose Cauchy point lies before every breakpoint, which a product decides (below): the common case
        const bool brk = moving & (neggi != 0.0);
        tbp[j] = brk ? (neggi < 0.0 ? tl : tu) : kInf;
        nbr += brk ? 1 : 0;
        z[j] = x[j];
      }
      // tbp[] holds numerators until this turns them into breakpoints (nine f64 divisions per lane)
      auto breakpoints = [&]() {
#pragma unroll
        for (int j = 0; j < J; ++j) tbp[j] = tbp[j] / fabs(g[j]);            // +inf / |g| stays +inf (|g| is finite); brk implies g != 0
      };
      SE3MPC_TICK(8)
      if (col == 0 && !q.seq_cauchy) {
        // No L-BFGS pairs yet: B = theta*I and the piecewise quadratic along the projected path is
        //   m(t) = sum_i g_i^2 (theta*tau_i^2/2 - tau_i),  tau_i = min(t, t_i),
        // whose derivative sum_{t_i > t} g_i^2 (theta*t - 1) is negative on [0, 1/theta): the sequential
        // search of the published algorithm (f1_k = -(D - S_k)(1 - theta*t_k), f2_k = theta*(D - S_k), hence
        // dtm_k = 1/theta - t_k at every breakpoint) crosses exactly the breakpoints t_i <= 1/theta and stops
        // at t = 1/theta.  This is where ~170 of a typical solve's ~172 crossings happen (all of them at
        // the first iterate), so they are taken in one parallel pass instead of 170 group reductions.
        if (sbgnrm > 0.0) {
          const double tstar = 1.0 / theta;
          const bool unit = theta == 1.0;                                  // the first iterate of every solve
          if (!unit) breakpoints();
#pragma unroll
          for (int j = 0; j < J; ++j) {
            // fl(num / |g|) <= 1 <=> num <= |g| (rounding is monotone and fl(1) = 1): no quotient while theta is 1
            const bool reached = unit ? tbp[j] <= fabs(g[j]) : tbp[j] <= tstar;
            const bool hit = (iwhere[j] == 0) & reached;                   // d is 0 wherever iwhere != 0: z + tstar*d leaves those alone
            const bool upw = d[j] > 0.0;
            z[j] = hit ? (upw ? box_hi(q, j) : box_lo(q, j)) : z[j] + tstar * d[j];
            iwhere[j] = hit ? (upw ? 2 : 1) : iwhere[j];
            d[j] = hit ? 0.0 : d[j];
          }
        }
        SE3MPC_TICK(9)
      } else {
      double f1 = group_sum<G>(f1p);
      const int nbreak = group_sum_i32<G>(nbr);
      // p = W'd (2col group reductions), second half scaled by theta
      for (int c = 0; c < col; ++c) {
        double a1 = 0.0, a2 = 0.0;
        IO w[2 * J];
        load_row(ROW(c), w);
#pragma unroll
        for (int j = 0; j < J; ++j) { a1 += (double)w[2 * j + 1] * d[j]; a2 += (double)w[2 * j] * d[j]; }
        double r2[2] = {a1, a2};
        group_sum_n<G, 2>(r2);
        a1 = r2[0]; a2 = r2[1];
        if (k == 0) { pv[c] = a1; pv[col + c] = theta * a2; cv[c] = 0.0; cv[col + c] = 0.0; }
      }
      group_sync<G>();
      if (sbgnrm > 0.0 && nbreak > 0) {
        double f2 = -theta * f1;
        const double f2_org = f2;
        if (col > 0 && col <= kFastCol) {
          auto init_fast = [&](auto tag) {
            constexpr int C = decltype(tag)::value;
            MidRegs<C> M;
            load_mid<C>(sy, wt, m, M);
            double v[2 * C], pr[2 * C];
#pragma unroll
            for (int i = 0; i < 2 * C; ++i) v[i] = pv[i];
            info = bmv_regs<C>(M, v, pr);
            double dot = 0.0;
#pragma unroll
            for (int i = 0; i < 2 * C; ++i) dot += pr[i] * v[i];
            f2 -= dot;
          };
          if (col == 1) init_fast(ColTag<1>{}); else init_fast(ColTag<2>{});
        } else if (col > 0) {
          if (k == 0) {
            const int inf = bmv(sy, wt, m, col, pv, vv);
            double dot = 0.0;
            for (int i = 0; i < 2 * col; ++i) dot += vv[i] * pv[i];
            sc[0] = dot; sc[1] = (double)inf;
          }
          group_sync<G>();
          info = (int)sc[1];
          f2 -= sc[0];
          group_sync<G>();
        }
        SE3MPC_TICK(10)
        if (info == 0) {
          double dtm = -f1 / f2, tsum = 0.0, tj = 0.0;
          int nleft = nbreak;
          bool all_fixed = false;
          // The search below stops before its first crossing when dtm < min_j t_j.  num * (1 - 2^-50) > dtm * |g| (both products rounded) implies
          // num / |g| > dtm * (1 + 2^-51), hence fl(num / |g|) > dtm: if that holds in every lane the loop would do nothing but form the nine
          // quotients per lane and their group minimum -- skipped.  Otherwise (a crossing, or too close to call) the published search runs.
          // (accumulated with `&`, not a short-circuit `&&` chain: straight-line compares instead of nine nested divergent regions)
          bool clear = dtm > 0.0;
#pragma unroll
          for (int j = 0; j < J; ++j) clear = clear & (tbp[j] * 0.99999999999999911182158029987 > dtm * fabs(g[j]));
          const bool skip_search = group_ballot<G>(!clear) == 0ull;
          if (!skip_search) breakpoints();
          while (!skip_search && nleft > 0) {
            // next smallest breakpoint: per-lane min, group min, owner = first lane holding it
            double tmin = tbp[0];
            int jm = 0;
#pragma unroll
            for (int j = 1; j < J; ++j) if (tbp[j] < tmin) { tmin = tbp[j]; jm = j; }
            const double tj0 = tj;
            tj = group_min<G>(tmin);
            const int src = first_lane(group_ballot<G>(tmin == tj));
            if (src < 0) { info = 1; break; }                 // NaN breakpoints: give up on this memory
            const int jsel = group_bcast<G>(jm, src);
            const double dt = tj - tj0;
            if (dtm < dt) break;
            tsum += dt;
            --nleft;
            SE3MPC_COUNT(15)
            // owner fixes its variable at the bound it hits
            double dib = 0.0, zib = 0.0;
#pragma unroll
            for (int j = 0; j < J; ++j) {
              if (j == jsel && k == src) {
                const double lo = box_lo(q, j), hi = box_hi(q, j);
                dib = d[j]; d[j] = 0.0; tbp[j] = kInf;
                if (dib > 0.0) { zib = hi - x[j]; z[j] = hi; iwhere[j] = 2; }
                else { zib = lo - x[j]; z[j] = lo; iwhere[j] = 1; }
              }
            }
            const double dibp = group_bcast<G>(dib, src), zibp = group_bcast<G>(zib, src);
            if (nleft == 0 && nbreak == n) { dtm = dt; all_fixed = true; break; }
            const double dibp2 = dibp * dibp;
            f1 = f1 + dt * f2 + dibp2 - theta * dibp * zibp;
            f2 = f2 - theta * dibp2;
            const int ibp = (lane - k + src) * LS + 2 * jsel;      // the owner's (s, y) couple inside a pair's [64][LS] image
            // (the middle-matrix product of a crossing runs as a scalar section of the group's first lane for every col: a crossing with
            // pairs in memory is rare -- none in a typical solve -- and its register form was one of the kernel's two pressure peaks)
            if (col > 0) {
              if (k == 0) {
                for (int i = 0; i < 2 * col; ++i) cv[i] += dt * pv[i];
                for (int c = 0; c < col; ++c) { wbp[c] = (double)pairs[c * kWave * LS + ibp + 1]; wbp[col + c] = theta * (double)pairs[c * kWave * LS + ibp]; }
                const int inf = bmv(sy, wt, m, col, wbp, vv);
                double wmc = 0.0, wmp = 0.0, wmw = 0.0;
                for (int i = 0; i < 2 * col; ++i) { wmc += cv[i] * vv[i]; wmp += pv[i] * vv[i]; wmw += wbp[i] * vv[i]; }
                for (int i = 0; i < 2 * col; ++i) pv[i] -= dibp * wbp[i];
                sc[0] = wmc; sc[1] = wmp; sc[2] = wmw; sc[3] = (double)inf;
              }
              group_sync<G>();
              info = (int)sc[3];
              f1 += dibp * sc[0];
              f2 += 2.0 * dibp * sc[1] - dibp2 * sc[2];
              group_sync<G>();
              if (info != 0) break;
            }
            f2 = fmax(kEps * f2_org, f2);
            if (nleft > 0) dtm = -f1 / f2;
            else { f1 = 0.0; f2 = 0.0; dtm = 0.0; }       // every variable with d != 0 has hit a bound
          }
          SE3MPC_TICK(11)
          if (info == 0) {
            if (!all_fixed) {
              if (dtm <= 0.0) dtm = 0.0;
              tsum += dtm;
#pragma unroll
              for (int j = 0; j < J; ++j) z[j] += tsum * d[j];
            }
            if (col > 0) {
              if (k == 0) for (int i = 0; i < 2 * col; ++i) cv[i] += dtm * pv[i];
              group_sync<G>();
            }
          }
        }
      }
      }   // col > 0: sequential search
    }
    if (info != 0) { col = 0; theta = 1.0; iupdat = 0; continue; }   // singular middle matrix: refresh memory

    SE3MPC_TICK(2)
    // ===================================================================== subspace minimization
    int nfree_p = 0;
#pragma unroll
    for (int j = 0; j < J; ++j) nfree_p += (iwhere[j] <= 0) ? 1 : 0;
    const int nfree = group_sum_i32<G>(nfree_p);
    if (nfree != 0 && col != 0) {
      // wvr: the subspace solution (K^-1 W'Z r) of the fast path, in registers of every lane; the LDS path leaves it in wv[]
      double wvr[2 * kFastCol] = {0.0, 0.0, 0.0, 0.0};
      if (col <= kFastCol) {
        auto subspace_fast = [&](auto tag) {
          constexpr int C = decltype(tag)::value;
          // ---- formk: the same inner products, accumulated into a register matrix (upper triangle of the 2C x 2C K matrix)
          double wnr[2 * C][2 * C];
#pragma unroll
          for (int i = 0; i < 2 * C; ++i)
#pragma unroll
            for (int kk = 0; kk < 2 * C; ++kk) wnr[i][kk] = 0.0;
          // all C*C cells' partial sums first, then ONE interleaved reduction of the 3 sums each cell needs (yzzy, saas for the
          // lower-left half, and the cross term: sa_y below the diagonal, sz_y on and above it)
          double sums[3 * C * C];
#pragma unroll
          for (int i = 0; i < 3 * C * C; ++i) sums[i] = 0.0;
          // (the rows of all C pairs are needed at once here: 18 C registers in the float kernel; the double kernel with two pairs would
          // need 72 and reads couple by couple instead -- 16 bytes per read there too)
          constexpr bool kRows = sizeof(IO) == 4 || C == 1;
          IO wr_[kRows ? C : 1][2 * J];
          if constexpr (kRows) {
#pragma unroll
            for (int c = 0; c < C; ++c) load_row(ROW(c), wr_[c]);
          }
#pragma unroll
          for (int j = 0; j < J; ++j) {                        // slot-outer: a slot's 2C values of S, Y are folded into every cell
            const bool fr = iwhere[j] <= 0;
            double wyv[C], wsv[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
              if constexpr (kRows) { wyv[c] = (double)wr_[c][2 * j + 1]; wsv[c] = (double)wr_[c][2 * j]; }
              else { wyv[c] = (double)WY(c, j); wsv[c] = (double)WS(c, j); }
            }
#pragma unroll
            for (int iy = 0; iy < C; ++iy) {
#pragma unroll
              for (int jy = 0; jy < C; ++jy) {
                const double yy = wyv[iy] * wyv[jy], sS = wsv[iy] * wsv[jy], sY = wsv[iy] * wyv[jy];
                sums[3 * (iy * C + jy) + 0] += fr ? yy : 0.0;                                  // yzzy: free set
                sums[3 * (iy * C + jy) + 1] += fr ? 0.0 : sS;                                  // saas: active set
                sums[3 * (iy * C + jy) + 2] += ((jy < iy) ? !fr : fr) ? sY : 0.0;              // sa_y below the diagonal, sz_y on and above it
              }
            }
          }
          group_sum_n<G, 3 * C * C>(sums);
#pragma unroll
          for (int iy = 0; iy < C; ++iy) {
#pragma unroll
            for (int jy = 0; jy < C; ++jy) {
              const double yzzy = sums[3 * (iy * C + jy) + 0], saas = sums[3 * (iy * C + jy) + 1], cross = sums[3 * (iy * C + jy) + 2];
              if (jy <= iy) {
                wnr[jy][iy] = yzzy / theta + (jy == iy ? sy[iy * m + iy] : 0.0);
                wnr[C + jy][C + iy] = saas * theta;
              }
              wnr[jy][C + iy] = (jy < iy) ? -cross : cross;
            }
          }
          reload_lds();
          int inf = formk_factor_regs<C>(wnr);
          SE3MPC_TICK(12)
          // ---- cmprlb, scalar part: mc = M c
          MidRegs<C> M;
          load_mid<C>(sy, wt, m, M);
          double cr[2 * C], mc[2 * C];
#pragma unroll
          for (int i = 0; i < 2 * C; ++i) cr[i] = cv[i];
          if (inf == 0 && bmv_regs<C>(M, cr, mc)) inf = -8;
          info = inf;
          if (info != 0) return;
          // ---- cmprlb: r = -Z'(B(xcp - x) + g)   (held in d[] on the free variables)
#pragma unroll
          for (int j = 0; j < J; ++j) d[j] = -theta * (z[j] - x[j]) - g[j];     // every variable's value first, ONE select at the end (d stays 0 off the free set)
#pragma unroll
          for (int c = 0; c < C; ++c) {                        // pair-outer: one row in registers at a time; per element the additions keep their order
            IO w[2 * J];
            load_row(ROW(c), w);
#pragma unroll
            for (int j = 0; j < J; ++j) d[j] += (double)w[2 * j + 1] * mc[c] + (double)w[2 * j] * (theta * mc[C + c]);
          }
#pragma unroll
          for (int j = 0; j < J; ++j) d[j] = (iwhere[j] <= 0) ? d[j] : 0.0;
          reload_lds();
          // ---- subsm: wv = W'Z d ; wv = K^-1 wv   (d is 0 off the free set: no condition inside the sums)
          double wr[2 * C];
#pragma unroll
          for (int c = 0; c < C; ++c) {
            double a1 = 0.0, a2 = 0.0;
            IO w[2 * J];
            load_row(ROW(c), w);
#pragma unroll
            for (int j = 0; j < J; ++j) { a1 += (double)w[2 * j + 1] * d[j]; a2 += (double)w[2 * j] * d[j]; }
            wr[c] = a1; wr[C + c] = a2;
          }
          group_sum_n<G, 2 * C>(wr);
#pragma unroll
          for (int c = 0; c < C; ++c) wr[C + c] = theta * wr[C + c];
          reload_lds();
          int inf2 = dtrsl_regs<2 * C>(wnr, wr, true);
          if (!inf2) {
#pragma unroll
            for (int i = 0; i < C; ++i) wr[i] = -wr[i];
            inf2 = dtrsl_regs<2 * C>(wnr, wr, false);
          }
          info = inf2;
#pragma unroll
          for (int i = 0; i < C; ++i) { wvr[i] = wr[i]; wvr[kFastCol + i] = wr[C + i]; }
        };
        if (col == 1) subspace_fast(ColTag<1>{}); else subspace_fast(ColTag<2>{});
      } else {
        // ---- formk: K blocks from inner products over the free (Z) and active (A) sets
        for (int iy = 0; iy < col; ++iy) {
          for (int jy = 0; jy < col; ++jy) {
            double yzzy = 0.0, saas = 0.0, sa_y = 0.0, sz_y = 0.0;
  #pragma unroll
            for (int j = 0; j < J; ++j) {
              const bool fr = iwhere[j] <= 0;
              const double wyi = (double)WY(iy, j), wyj = (double)WY(jy, j), wsi = (double)WS(iy, j), wsj = (double)WS(jy, j);
              if (fr) { yzzy += wyi * wyj; sz_y += wsi * wyj; }
              else { saas += wsi * wsj; sa_y += wsi * wyj; }     // active set (padding rows of S, Y are zero)
            }
            // wn (upper triangle, row stride 2m):  [ D + Y'ZZ'Y/theta   -L_a' + R_z' ;  .   theta S'AA'S ]
            if (jy <= iy) {
              yzzy = group_sum<G>(yzzy); saas = group_sum<G>(saas);
              if (k == 0) {
                wn[jy * 2 * m + iy] = yzzy / theta + (jy == iy ? sy[iy * m + iy] : 0.0);
                wn[(col + jy) * 2 * m + (col + iy)] = saas * theta;
              }
            }
            if (jy < iy) {
              sa_y = group_sum<G>(sa_y);
              if (k == 0) wn[jy * 2 * m + (col + iy)] = -sa_y;
            } else {
              sz_y = group_sum<G>(sz_y);
              if (k == 0) wn[jy * 2 * m + (col + iy)] = sz_y;
            }
          }
        }
        group_sync<G>();
        if (k == 0) {
          const int ld = 2 * m;
          int inf = dpofa(wn, ld, col);
          if (inf) inf = -1;
          else {
            for (int js = col; js < 2 * col; ++js) dtrsl_upper(wn, ld, col, wn + js, ld, true);
            for (int is = col; is < 2 * col; ++is)
              for (int js = is; js < 2 * col; ++js) {
                double s = 0.0;
                for (int kk = 0; kk < col; ++kk) s += wn[kk * ld + is] * wn[kk * ld + js];
                wn[is * ld + js] += s;
              }
            if (dpofa(wn + col * ld + col, ld, col)) inf = -2;
          }
          // ---- cmprlb, scalar part: mc = M c
          if (inf == 0 && bmv(sy, wt, m, col, cv, vv)) inf = -8;
          sc[0] = (double)inf;
        }
        group_sync<G>();
        info = (int)sc[0];
        if (info == 0) {
          // ---- cmprlb: r = -Z'(B(xcp - x) + g)   (held in d[] on the free variables)
  #pragma unroll
          for (int j = 0; j < J; ++j) d[j] = (iwhere[j] <= 0) ? (-theta * (z[j] - x[j]) - g[j]) : 0.0;
          for (int c = 0; c < col; ++c) {
            const double a1 = vv[c], a2 = theta * vv[col + c];
  #pragma unroll
            for (int j = 0; j < J; ++j) if (iwhere[j] <= 0) d[j] += (double)WY(c, j) * a1 + (double)WS(c, j) * a2;
          }
          // ---- subsm: wv = W'Z d ; wv = K^-1 wv ; d = (d + Z'W wv-ish)/theta
          for (int c = 0; c < col; ++c) {
            double a1 = 0.0, a2 = 0.0;
  #pragma unroll
            for (int j = 0; j < J; ++j) if (iwhere[j] <= 0) { a1 += (double)WY(c, j) * d[j]; a2 += (double)WS(c, j) * d[j]; }
            double r2[2] = {a1, a2};
            group_sum_n<G, 2>(r2);
            a1 = r2[0]; a2 = r2[1];
            if (k == 0) { wv[c] = a1; wv[col + c] = theta * a2; }
          }
          group_sync<G>();
          if (k == 0) {
            int inf = dtrsl_upper(wn, 2 * m, 2 * col, wv, 1, true);
            if (!inf) {
              for (int i = 0; i < col; ++i) wv[i] = -wv[i];
              inf = dtrsl_upper(wn, 2 * m, 2 * col, wv, 1, false);
            }
            sc[0] = (double)inf;
          }
          group_sync<G>();
          info = (int)sc[0];
        }
      }   // col > kFastCol: LDS path
      {
        if (info == 0) {
          if (col <= kFastCol) {
#pragma unroll
            for (int c = 0; c < kFastCol; ++c) {
              if (c < col) {
                const double b1 = wvr[c] / theta, b2 = wvr[kFastCol + c];
                IO w[2 * J];
                load_row(ROW(c), w);
#pragma unroll
                for (int j = 0; j < J; ++j) {
                  const double t = d[j] + ((double)w[2 * j + 1] * b1 + (double)w[2 * j] * b2);
                  d[j] = (iwhere[j] <= 0) ? t : d[j];
                }
              }
            }
          } else {
            for (int c = 0; c < col; ++c) {
              const double b1 = wv[c] / theta, b2 = wv[col + c];
#pragma unroll
              for (int j = 0; j < J; ++j) if (iwhere[j] <= 0) d[j] += (double)WY(c, j) * b1 + (double)WS(c, j) * b2;
            }
          }
          const double rth = 1.0 / theta;
          // projected Newton point; xo is free here (the line search re-saves it): xo keeps xcp
          bool hitp = false;
          double ddp = 0.0;
#pragma unroll
          for (int j = 0; j < J; ++j) {
            xo[j] = z[j];
            const bool fr = iwhere[j] <= 0;
            const double lo = box_lo(q, j), hi = box_hi(q, j);
            const double dn = d[j] * rth;
            const double xk = fmin(hi, fmax(lo, z[j] + dn));
            d[j] = fr ? dn : d[j];
            z[j] = fr ? xk : z[j];
            hitp = hitp | (fr & ((xk == lo) | (xk == hi)));
            ddp += (z[j] - x[j]) * g[j];
          }
          const bool iword = group_ballot<G>(hitp) != 0ull;
          if (iword) {
            const double dd_p = group_sum<G>(ddp);
            if (dd_p > 0.0) {
              // not a descent direction: back to xcp and truncate the Newton step at the first bound
              double amin = 1.0;
              unsigned imin = 0xFFFFFFFFu;
#pragma unroll
              for (int j = 0; j < J; ++j) {
                z[j] = xo[j];
                if (iwhere[j] <= 0) {
                  const double lo = box_lo(q, j), hi = box_hi(q, j);
                  const double dk = d[j];
                  double cand = 1.0;
                  if (dk < 0.0) { const double t2 = lo - z[j]; cand = (t2 >= 0.0) ? 0.0 : ((dk * 1.0 < t2) ? t2 / dk : 1.0); }
                  else if (dk > 0.0) { const double t2 = hi - z[j]; cand = (t2 <= 0.0) ? 0.0 : ((dk * 1.0 > t2) ? t2 / dk : 1.0); }
                  // ties go to the variable that comes first in the reference's packing [P | V | T], row = 3k + axis (subsm's strict `<` in variable order):
                  // inside a lane the slots are visited in that order, across lanes the smallest index wins below
                  const unsigned idx = (unsigned)((j / 3) * n3 + 3 * k + (j % 3));
                  if (cand < amin) { amin = cand; imin = idx; }
                }
              }
              const double alpha = group_min<G>(amin);
              const unsigned ibd = group_min_u32<G>(amin == alpha && alpha < 1.0 ? imin : 0xFFFFFFFFu);
#pragma unroll
              for (int j = 0; j < J; ++j) {
                if (iwhere[j] <= 0) {
                  const unsigned idx = (unsigned)((j / 3) * n3 + 3 * k + (j % 3));
                  if (alpha < 1.0 && idx == ibd) {
                    if (d[j] > 0.0) { z[j] = box_hi(q, j); d[j] = 0.0; }
                    else if (d[j] < 0.0) { z[j] = box_lo(q, j); d[j] = 0.0; }
                  }
                  z[j] += alpha * d[j];
                }
              }
            }
          }
        }
      }
      if (info != 0) { col = 0; theta = 1.0; iupdat = 0; continue; }
    }

    SE3MPC_TICK(3)
    // ===================================================================== line search (lnsrlb)
    double dtdp = 0.0, gd0p = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) { d[j] = z[j] - x[j]; dtdp += d[j] * d[j]; gd0p += g[j] * d[j]; }
    double r2[2] = {dtdp, gd0p};
    group_sum_n<G, 2>(r2);
    const double dtd = r2[0];
    gd_fused = r2[1];                                         // g'd at the start of the search
    double stpmx;
    if (iter == 0) stpmx = 1.0;
    else {
      double smx = kBig;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const double lo = box_lo(q, j), hi = box_hi(q, j);
        const double a1 = d[j];
        const bool neg = a1 < 0.0, pos = a1 > 0.0;
        const double a2 = neg ? lo - x[j] : hi - x[j];
        const bool blocked = neg ? a2 >= 0.0 : (pos & (a2 <= 0.0));
        const bool tighter = neg ? a1 * smx < a2 : (pos & (a1 * smx > a2));
        const double quot = a2 / a1;
        smx = blocked ? 0.0 : (tighter ? quot : smx);
      }
      stpmx = group_min<G>(smx);
    }
    double stp = 1.0;
#pragma unroll
    for (int j = 0; j < J; ++j) xo[j] = opaque(x[j]);
    SE3MPC_TICK(13)
    fold = f;
    int ifun = 0, iback = 0, ls_info = 0;
    double gd = 0.0, gdold = 0.0;
    LineSearch ls;
    bool start = true;
    while (true) {
      gd = gd_fused;                                          // reduced together with dtd (first pass) or with f (after an evaluation)
      if (ifun == 0) {
        gdold = gd;
        if (gd >= 0.0) { ls_info = -4; break; }
      }
      const int lt = dcsrch(f, gd, stp, 0.0, stpmx, start, ls);
      start = false;
      if (lt == LS_CONV || lt == LS_WARN) break;
      if (lt == LS_ERROR) { ls_info = -4; break; }          // dcsrch rejected its inputs (never with a feasible d)
      ++ifun; iback = ifun - 1;
      if (iback >= q.maxls) break;
      // the trial point; `moved`: it differs from the x of the last evaluation (which the registers still hold)
      bool moved = false;
      if (stp == 1.0) {
#pragma unroll
        for (int j = 0; j < J; ++j) { moved = moved | !(z[j] == x[j]); x[j] = z[j]; }
      } else {
#pragma unroll
        for (int j = 0; j < J; ++j) { const double xn = stp * (z[j] - xo[j]) + xo[j]; moved = moved | !(xn == x[j]); x[j] = xn; }
      }
      if (!x_is_last || group_ballot<G>(moved) != 0ull) ++nfev;
      x_is_last = true;
      SE3MPC_TICK(4)
      f = eval_fg(true);
      SE3MPC_TICK(1)
    }
    SE3MPC_TICK(4)
    if (ls_info != 0 || iback >= q.maxls) {
      // restore the previous iterate (its gradient recomputed).  x held the x of the last evaluation, or the iterate itself when
      // this search evaluated nothing; after the restore it still does only if the two are the same point.
      bool differs = false;
#pragma unroll
      for (int j = 0; j < J; ++j) { differs = differs | !(x[j] == xo[j]); x[j] = xo[j]; g[j] = grad_of(j, xo[j]); }     // (g was not touched by the search: this is what it holds already, bit for bit)
      if (group_ballot<G>(differs) != 0ull) x_is_last = false;
      f = fold;
      // (SciPy reports a stop past one of its limits as status 1 whatever the task says: warnflag = 1 when nfev > maxfun or nit >= maxiter)
      if (col == 0) { task = SE3MPC_TASK_ABNORMAL; status = (nfev > q.maxfun || nit >= q.maxiter) ? 1 : 2; break; }
      col = 0; theta = 1.0; iupdat = 0;
      continue;
    }

    // ===================================================================== new iterate
    ++iter; ++nit;
#pragma unroll
    for (int j = 0; j < J; ++j) g[j] = grad_of(j, x[j]);      // the gradient at the accepted point (the search's evaluations did not store it)
    sbgnrm = projgr();
    if (nit >= q.maxiter) { task = SE3MPC_TASK_STOP_MAXITER; status = 1; break; }
    if (nfev > q.maxfun) { task = SE3MPC_TASK_STOP_MAXFUN; status = 1; break; }
    if (sbgnrm <= q.pgtol) { task = SE3MPC_TASK_CONV_PGTOL; status = 0; break; }
    {
      const double ddum = fmax(fabs(fold), fmax(fabs(f), 1.0));
      if ((fold - f) <= q.ftol * ddum) { task = SE3MPC_TASK_CONV_FTOL; status = 0; break; }
    }
    // ---- BFGS update (matupd + formt); d is formed again from x_old, then xo becomes y = g - g(x_old)
    double rrp = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) { d[j] = z[j] - xo[j]; xo[j] = g[j] - grad_of(j, xo[j]); rrp += xo[j] * xo[j]; }
    const double rr = group_sum<G>(rrp);
    double dr, ddum;
    if (stp == 1.0) { dr = gd - gdold; ddum = -gdold; }
    else {
      dr = (gd - gdold) * stp; ddum = -gdold * stp;
#pragma unroll
      for (int j = 0; j < J; ++j) d[j] *= stp;
    }
    if (dr <= kEps * ddum) continue;                    // skip the update
    ++iupdat;
    if (iupdat > m && m < q.m) { task = SE3MPC_TASK_OVERFLOW; status = 1; break; }   // second tier re-solves this problem
    if (iupdat <= m) col = iupdat;
    else {
      // memory full: drop the oldest pair (each lane shifts its own elements; the first lane the small matrices)
      for (int c = 0; c + 1 < m; ++c) {
#pragma unroll
        for (int j = 0; j < J; ++j) { WS(c, j) = WS(c + 1, j); WY(c, j) = WY(c + 1, j); }
      }
      if (k == 0)
        for (int i = 0; i + 1 < m; ++i)
          for (int kk = 0; kk + 1 < m; ++kk) { ss[i * m + kk] = ss[(i + 1) * m + kk + 1]; sy[i * m + kk] = sy[(i + 1) * m + kk + 1]; }
      group_sync<G>();
    }
    { IO w[2 * J];
#pragma unroll
      for (int j = 0; j < J; ++j) { w[2 * j] = (IO)d[j]; w[2 * j + 1] = (IO)xo[j]; }
      store_row(ROW(col - 1), w); }
    theta = rr / dr;
    bool formt_failed;
    if (col <= kFastCol) {
      // matupd's new row / column and formt on registers: every lane forms theta*S'S + L D^-1 L' and its Cholesky factor from
      // group-uniform values; the first lane writes the state (sy, ss, wt) back for the next iteration
      auto update_fast = [&](auto tag) {
        constexpr int C = decltype(tag)::value;
        double syr[C][C], ssr[C][C], wtr[C][C];
#pragma unroll
        for (int i = 0; i < C; ++i)
#pragma unroll
          for (int kk = 0; kk < C; ++kk) { syr[i][kk] = (kk <= i && i < C - 1) ? sy[i * m + kk] : 0.0; ssr[i][kk] = (kk >= i && kk < C - 1) ? ss[i * m + kk] : 0.0; wtr[i][kk] = 0.0; }
#pragma unroll
        for (int c = 0; c + 1 < C; ++c) {
          double a1 = 0.0, a2 = 0.0;
          IO w[2 * J];
          load_row(ROW(c), w);
#pragma unroll
          for (int j = 0; j < J; ++j) { a1 += d[j] * (double)w[2 * j + 1]; a2 += (double)w[2 * j] * d[j]; }
          double r2[2] = {a1, a2};
          group_sum_n<G, 2>(r2);
          syr[C - 1][c] = r2[0]; ssr[c][C - 1] = r2[1];
        }
        ssr[C - 1][C - 1] = (stp == 1.0) ? dtd : stp * stp * dtd;
        syr[C - 1][C - 1] = dr;
        // formt: T = theta*S'S + L D^-1 L', Cholesky factor in wt
#pragma unroll
        for (int jj = 0; jj < C; ++jj) wtr[0][jj] = theta * ssr[0][jj];
#pragma unroll
        for (int i = 1; i < C; ++i)
#pragma unroll
          for (int jj = i; jj < C; ++jj) {
            const int k1 = i < jj ? i : jj;
            double dd = 0.0;
#pragma unroll
            for (int kk = 0; kk < C; ++kk) if (kk < k1) dd += syr[i][kk] * syr[jj][kk] / syr[kk][kk];
            wtr[i][jj] = dd + theta * ssr[i][jj];
          }
        formt_failed = dpofa_regs<C, 0, C>(wtr) != 0;
        group_sync<G>();
        if (k == 0) {
#pragma unroll
          for (int c = 0; c < C; ++c) { sy[(C - 1) * m + c] = syr[C - 1][c]; ss[c * m + (C - 1)] = ssr[c][C - 1]; }
#pragma unroll
          for (int i = 0; i < C; ++i)
#pragma unroll
            for (int jj = 0; jj < C; ++jj) if (jj >= i) wt[i * m + jj] = wtr[i][jj];
        }
        group_sync<G>();
      };
      if (col == 1) update_fast(ColTag<1>{}); else update_fast(ColTag<2>{});
    } else {
      for (int c = 0; c + 1 < col; ++c) {
        double a1 = 0.0, a2 = 0.0;
  #pragma unroll
        for (int j = 0; j < J; ++j) { a1 += d[j] * (double)WY(c, j); a2 += (double)WS(c, j) * d[j]; }
        a1 = group_sum<G>(a1); a2 = group_sum<G>(a2);
        if (k == 0) { sy[(col - 1) * m + c] = a1; ss[c * m + (col - 1)] = a2; }
      }
      if (k == 0) {
        ss[(col - 1) * m + (col - 1)] = (stp == 1.0) ? dtd : stp * stp * dtd;
        sy[(col - 1) * m + (col - 1)] = dr;
        // formt: T = theta*S'S + L D^-1 L', Cholesky factor in wt
        for (int jj = 0; jj < col; ++jj) wt[jj] = theta * ss[jj];
        for (int i = 1; i < col; ++i)
          for (int jj = i; jj < col; ++jj) {
            const int k1 = i < jj ? i : jj;
            double dd = 0.0;
            for (int kk = 0; kk < k1; ++kk) dd += sy[i * m + kk] * sy[jj * m + kk] / sy[kk * m + kk];
            wt[i * m + jj] = dd + theta * ss[i * m + jj];
          }
        sc[0] = (double)dpofa(wt, m, col);
      }
      group_sync<G>();
      formt_failed = sc[0] != 0.0;
      group_sync<G>();
    }
    if (formt_failed) { col = 0; theta = 1.0; iupdat = 0; }

  }

