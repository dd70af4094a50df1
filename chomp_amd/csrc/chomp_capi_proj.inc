// HaloFit + projection entry points (included inside extern "C" of chomp_capi.hip).

// The two launches of a HaloFit set-up (halo.py:1261-1317) on the context's current stream.
static int halofit_launch(chomp_ctx* ctx, size_t dst, size_t src, double f_1, double f_2,
                          double f_3, double omega_l, double w) {
  const TabLayout& L = ctx->L;
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_halofit_sigma<BAO>, dim3(L.NK), dim3(256), 0, ctx->stream, ctx->cfg, L,
                       ctx->d_epochs, (int)src, ctx->d_tab);
  });
  hipLaunchKernelGGL(k_halofit_finalize, dim3(1), dim3(64),
                     (size_t)(25 * L.NK + 64) * sizeof(double), ctx->stream, L, ctx->d_epochs,
                     (int)dst, (int)src, ctx->d_tab, f_1, f_2, f_3, omega_l, w, ctx->d_hf_ainv);
  HIPCHK(hipGetLastError());
  ctx->have_halofit[dst] = 1;
  return CHOMP_OK;
}

int chomp_halofit_setup(chomp_ctx* ctx, size_t dst, size_t src, double f_1, double f_2,
                        double f_3, double omega_l, double w) {
  StageRange range_(ctx, "chomp:halofit_setup");
  if (!ctx) return CHOMP_ERR_ARG;
  if (!ctx->have_mass) return fail(ctx, CHOMP_ERR_STATE, "halofit_setup before mass_setup");
  if (dst >= ctx->n_epoch || src >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_ARG, "halofit_setup: epoch");
  HIPCHK(hipSetDevice(ctx->device));
  return halofit_launch(ctx, dst, src, f_1, f_2, f_3, omega_l, w);
}

// chomp_stage_k and chomp_halofit_setup(epoch, epoch, ...) in one call.  HaloFit's sigma table
// and fit (47 us, the fit a single wavefront) need the epoch record as the mass function left
// it and nothing of the halo model's knot integrals, which need nothing of HaloFit: behind
// k_mass_nodes -- the last kernel that rewrites the whole record -- the two run side by side,
// HaloFit on the side stream, joined before the call returns.
int chomp_stage_k_halofit(chomp_ctx* ctx, const chomp_halo_par* mass_par, int mf_kind,
                          const chomp_halo_par* profile, const chomp_hod_par* hod,
                          unsigned tables, size_t epoch, double f_1, double f_2, double f_3,
                          double omega_l, double w) {
  if (!ctx || !mass_par || !profile || !hod) return fail(ctx, CHOMP_ERR_ARG, "stage_k_halofit: bad args");
  const std::vector<chomp_hod_model> m = zheng_models(hod, ctx->n_epoch);
  return chomp_stage_k_halofit_hod(ctx, mass_par, mf_kind, profile, m.data(), tables, epoch, f_1,
                                   f_2, f_3, omega_l, w);
}

int chomp_stage_k_halofit_hod(chomp_ctx* ctx, const chomp_halo_par* mass_par, int mf_kind,
                              const chomp_halo_par* profile, const chomp_hod_model* hod,
                              unsigned tables, size_t epoch, double f_1, double f_2,
                              double f_3, double omega_l, double w) {
  StageRange range_(ctx, "chomp:stage_k_halofit");
  if (!ctx || !mass_par || !profile || !hod) return fail(ctx, CHOMP_ERR_ARG, "stage_k_halofit: bad args");
  if (!ctx->have_epochs) return fail(ctx, CHOMP_ERR_STATE, "stage_k_halofit before epochs_set");
  if (epoch >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_ARG, "stage_k_halofit: epoch");
  if (mf_kind != CHOMP_MF_ST && mf_kind != CHOMP_MF_TINKER)
    return fail(ctx, CHOMP_ERR_ARG, "stage_k_halofit: unknown mass function kind");
  HIPCHK(hipSetDevice(ctx->device));
  int rc = upload(ctx, ctx->d_mass_par, mass_par, ctx->n_epoch * sizeof(chomp_halo_par));
  if (rc) return rc;
  HaloPlan P;
  rc = halo_prepare(ctx, profile, hod, tables, &P);
  if (rc) return rc;
  const HaloPlan Q = P.general ? constants_only(P) : P;
  if (!P.general) std::fill(ctx->prof_general.begin(), ctx->prof_general.end(), 0);
  rc = launch_nu_mass(ctx, mf_kind, &Q);
  if (rc) return rc;
  ctx->have_mass = true;
  bool forked = false;
  {
    SideScope side(ctx, &ctx->ev_side_done);
    rc = side.begin();
    if (rc) return rc;
    forked = side.on();
    rc = halofit_launch(ctx, epoch, epoch, f_1, f_2, f_3, omega_l, w);
  }
  const int rck = rc ? rc : (P.general ? launch_halo_general(ctx, P, profile) : launch_halo_knots(ctx, P));
  if (forked) HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_side_done, 0));
  return rck;
}

// n-th positive zero of J_order (scipy.special.jn_zeros(order, n)[-1],
// kernel.py:628-629, 806-807): McMahon's estimate bracketed and bisected on the
// same Chebyshev Bessel implementation the kernels use.
static double bessel_zero_host(int order, int n) {
  SiCiTab s;
  BesselTab j0, j2;
  fill_tables(&s, &j0, &j2);
  auto J = [&](double x) { return order == 0 ? bessel_j<0>(x, j0) : bessel_j<2>(x, j2); };
  const double beta = (n + 0.5 * order - 0.25) * M_PI;
  double lo = beta - 0.6, hi = beta + 0.6;
  double flo = J(lo);
  for (int it = 0; it < 200; ++it) {
    const double mid = 0.5 * (lo + hi);
    const double fm = J(mid);
    if ((fm < 0) == (flo < 0)) { lo = mid; flo = fm; } else { hi = mid; }
    if (hi - lo < 4e-16 * mid) break;
  }
  return 0.5 * (lo + hi);
}

// The projection set-up's pressure table, when its cosmology has w0-wa dark energy (queued
// on the stream in effect: the side stream), and the view its kernels evaluate E0 with.
static int proj_dark_energy(chomp_ctx* ctx, const chomp_cosmo* cosmo, DeSpline* view) {
  ProjState& P = ctx->proj;
  P.de = has_dark_energy(cosmo->w0, cosmo->wa);
  *view = DeSpline{nullptr, nullptr, 0};
  if (!P.de) return CHOMP_OK;
  const int rc = de_build(ctx, ctx->de_proj, std::vector<DePar>{DePar{cosmo->w0, cosmo->wa}});
  if (rc) { P.de = false; return rc; }
  *view = de_spline(ctx->de_proj.d_tab, ctx->cfg.cosmo_npoints);
  return CHOMP_OK;
}

// What chomp_kernel_setup and chomp_kernel_setup_sets validate alike (who: the caller's name).
static int proj_check_args(chomp_ctx* ctx, const char* who, double ktheta_min, double ktheta_max,
                           const chomp_window* const ws[2]) {
  const std::string w_ = std::string(who) + ": ";
  if (!(ktheta_min > 0.0) || !(ktheta_max > ktheta_min)) return fail(ctx, CHOMP_ERR_ARG, w_ + "ktheta range");
  for (int w = 0; w < 2; ++w) {
    if (ws[w]->kind < CHOMP_WINDOW_GALAXY || ws[w]->kind > CHOMP_WINDOW_CONVERGENCE_DELTA)
      return fail(ctx, CHOMP_ERR_SCOPE, w_ + "unknown window kind");
    const chomp_dndz& dz = ws[w]->dist;
    if (dz.kind != CHOMP_DNDZ_MAGLIM && dz.kind != CHOMP_DNDZ_GAUSSIAN &&
        dz.kind != CHOMP_DNDZ_BOXCAR && dz.kind != CHOMP_DNDZ_PPOLY)
      return fail(ctx, CHOMP_ERR_SCOPE, w_ + "only dNdz / dNdzMagLim / dNdzGaussian / "
                                             "dNdzInterpolation are in scope");
    if (dz.kind == CHOMP_DNDZ_PPOLY) {
      if (!dz.pp_breaks || !dz.pp_coef || dz.pp_n < 1 || dz.pp_n > 65536 || dz.pp_order < 0 ||
          dz.pp_order > 5)
        return fail(ctx, CHOMP_ERR_ARG, w_ + "dNdzInterpolation spline (pieces / order)");
      for (int i = 0; i < dz.pp_n; ++i)
        if (!(dz.pp_breaks[i + 1] > dz.pp_breaks[i]))
          return fail(ctx, CHOMP_ERR_ARG, w_ + "dNdzInterpolation breaks must increase");
    }
  }
  return CHOMP_OK;
}

// The ProjDev block of one set-up as the host prepares it (the device fills in the rest: norms,
// ranges, z_bar).  A tabulated distribution's table is the caller's to add (pp, pp_n, pp_order).
static ProjDev proj_host_block(const chomp_config& c, const chomp_cosmo* cosmo, double me_z_min,
                               double me_z_max, double ktheta_min, double ktheta_max,
                               const chomp_window* const ws[2], int bessel_order, double j_limit) {
  ProjDev pd;
  std::memset(&pd, 0, sizeof(pd));
  pd.om0 = cosmo->omega_m0; pd.ol0 = cosmo->omega_l0; pd.or0 = cosmo->omega_r0;
  pd.H0 = 100.0 / (2.998 * 100000.0);
  pd.growth_norm = growth_approx(pd.om0, pd.ol0, 1.0);
  pd.me_z_min[0] = me_z_min < 0.0 ? 0.0 : me_z_min;          // cosmology.py:748-750
  pd.me_z_max[0] = me_z_max;
  for (int w = 0; w < 2; ++w) {
    const chomp_window& W = *ws[w];
    pd.wkind[w] = W.kind;
    pd.dist[w].kind = W.dist.kind;
    pd.dist[w].z_min = W.dist.z_min;
    pd.dist[w].z_max = W.dist.z_max;
    for (int q = 0; q < 4; ++q) pd.dist[w].p[q] = W.dist.p[q];
    pd.dist[w].norm = 1.0;
    // WindowFunction.__init__ (kernel.py:234-240); Convergence spans [0, z_max] (:436)
    double zmin = (W.kind == CHOMP_WINDOW_GALAXY || W.kind == CHOMP_WINDOW_FLAT_CONVERGENCE)
                      ? W.dist.z_min : 0.0;
    if (zmin < c.window_precision) zmin = c.window_precision;
    pd.w_z_min[w] = zmin;
    pd.w_z_max[w] = W.dist.z_max;
    pd.me_z_min[w + 1] = zmin < 0.0 ? 0.0 : zmin;
    pd.me_z_max[w + 1] = W.dist.z_max;
  }
  pd.ln_kt_min = std::log(ktheta_min);
  pd.ln_kt_max = std::log(ktheta_max);
  pd.order = bessel_order;
  pd.j_limit = j_limit;
  return pd;
}

int chomp_kernel_setup(chomp_ctx* ctx, const chomp_cosmo* cosmo, double me_z_min,
                       double me_z_max, double ktheta_min, double ktheta_max,
                       const chomp_window* a, const chomp_window* b, int bessel_order) {
  StageRange range_(ctx, "chomp:kernel_setup (projection: MultiEpoch, windows, kernel knots)");
  if (!ctx || !cosmo || !a || !b) return fail(ctx, CHOMP_ERR_ARG, "kernel_setup: bad args");
  if (bessel_order != 0 && bessel_order != 2) return fail(ctx, CHOMP_ERR_ARG, "kernel_setup: bessel order must be 0 or 2");
  if (!ctx->dark_energy && has_dark_energy(cosmo->w0, cosmo->wa))
    return fail(ctx, CHOMP_ERR_SCOPE, "kernel_setup: w0/wa != -1/0 needs chomp_set_dark_energy(ctx, 1)");
  const chomp_window* ws[2] = {a, b};
  { const int rcc = proj_check_args(ctx, "kernel_setup", ktheta_min, ktheta_max, ws); if (rcc) return rcc; }
  HIPCHK(hipSetDevice(ctx->device));
  // On the side stream (SideScope): behind everything the context's stream holds now -- the
  // readers of the previous tables -- and beside whatever is queued there next (a halo set-up:
  // Correlation._prepare calls this first); the first reader joins (proj_join).
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  SideScope side(ctx, &ctx->ev_proj_ready, true);
  { const int rcs = side.begin(); if (rcs) return rcs; }
  const chomp_config& c = ctx->cfg;
  ProjState& P = ctx->proj;
  P.ready = false;
  P.me_ready = false;
  P.cov_ready = false;
  P.ssc_ready = false;
  P.ssc_prep = false;
  P.ng_ready = false;
  P.ng_prep = false;
  P.L = make_proj_layout(c.cosmo_npoints, c.window_npoints, c.kernel_npoints);
  // tabulated redshift distributions ride behind the projection tables
  size_t pp_doubles[2] = {0, 0};
  for (int w = 0; w < 2; ++w)
    if (ws[w]->dist.kind == CHOMP_DNDZ_PPOLY)
      pp_doubles[w] = (size_t)ws[w]->dist.pp_n * (ws[w]->dist.pp_order + 2) + 1;
  HIPCHK((hipError_t)P.d_pd.once(1));
  HIPCHK((hipError_t)P.d_pd_init.once(1));
  {   // (kept across calls: a free / malloc pair would drain the device on every set-up)
    bool moved = false;
    const int rce = ensure(ctx, P.d_tab, (size_t)P.L.total + pp_doubles[0] + pp_doubles[1], &moved);
    if (rce) return rce;
    // (the tabulated distributions' place behind the tables moves with the buffer and the
    //  layout: only then do they have to be sent again)
    if (moved || P.pp_total != (size_t)P.L.total + pp_doubles[0]) {
      ctx->sh_pp[0].reset();
      ctx->sh_pp[1].reset();
    }
    P.pp_total = (size_t)P.L.total + pp_doubles[0];
  }
  ProjDev pd = proj_host_block(c, cosmo, me_z_min, me_z_max, ktheta_min, ktheta_max, ws, bessel_order,
                               bessel_zero_host(bessel_order, c.kernel_bessel_limit));
  for (int w = 0; w < 2; ++w) {
    const chomp_window& W = *ws[w];
    if (W.dist.kind != CHOMP_DNDZ_PPOLY) continue;
    double* dst = P.d_tab + P.L.total + (w == 1 ? pp_doubles[0] : 0);
    const size_t nb = (size_t)W.dist.pp_n + 1, nc = (size_t)W.dist.pp_n * (W.dist.pp_order + 1);
    std::vector<double> blk(nb + nc);
    std::memcpy(blk.data(), W.dist.pp_breaks, nb * sizeof(double));
    std::memcpy(blk.data() + nb, W.dist.pp_coef, nc * sizeof(double));
    const int rcp = upload(ctx, dst, blk.data(), (nb + nc) * sizeof(double), ctx->sh_pp[w]);
    if (rcp) return rcp;
    pd.dist[w].pp = dst;
    pd.dist[w].pp_n = W.dist.pp_n;
    pd.dist[w].pp_order = W.dist.pp_order;
  }
  // (the device fills in the rest of the block -- norms, ranges, z_bar -- so every set-up starts
  //  from the block as the host prepared it: kept on the device, sent only when it changes, and
  //  copied into place on the stream -- a node of the graph under stream capture)
  { const int rcp = upload(ctx, P.d_pd_init, &pd, sizeof(pd), ctx->sh_proj); if (rcp) return rcp; }
  HIPCHK(hipMemcpyAsync(P.d_pd, P.d_pd_init, sizeof(pd), hipMemcpyDeviceToDevice, ctx->stream));
  P.host = pd;                      // (order, limits: what the host needs before kernel_info)
  const ProjLayout& L = P.L;
  if (L.NC > 240 || L.NWp > 360 || L.NKT > 720)          // (the spline builds are staged in 64 KB of LDS)
    return fail(ctx, CHOMP_ERR_ARG, "kernel_setup: cosmo/window/kernel_npoints too large");
  DeSpline de;
  { const int rcd = proj_dark_energy(ctx, cosmo, &de); if (rcd) return rcd; }
  if (P.de)
    hipLaunchKernelGGL(k_proj_chi<true>, dim3(L.NC, 4), dim3(64), 0, ctx->stream, c, L, P.d_pd, P.d_tab, de);
  else
    hipLaunchKernelGGL(k_proj_chi<false>, dim3(L.NC, 4), dim3(64), 0, ctx->stream, c, L, P.d_pd, P.d_tab, de);
  hipLaunchKernelGGL(k_proj_me_splines, dim3(3), dim3(192), (size_t)(33 * L.NC) * sizeof(double),
                     ctx->stream, c, L, P.d_pd, P.d_tab);
  if (P.de)
    hipLaunchKernelGGL(k_proj_window<true>, dim3(L.NWp, 2), dim3(64),
                       (size_t)(L.NC + 4 * (L.NC - 1)) * sizeof(double), ctx->stream, c, L, P.d_pd,
                       P.d_tab, de);
  else
    hipLaunchKernelGGL(k_proj_window<false>, dim3(L.NWp, 2), dim3(64),
                       (size_t)(L.NC + 4 * (L.NC - 1)) * sizeof(double), ctx->stream, c, L, P.d_pd,
                       P.d_tab, de);
  hipLaunchKernelGGL(k_proj_window_splines, dim3(1), dim3(128),
                     (size_t)(22 * L.NWp) * sizeof(double), ctx->stream, c, L, P.d_pd, P.d_tab);
  hipLaunchKernelGGL(k_proj_kernel_knots, dim3(L.NKT), dim3(256),
                     (size_t)ProjLds::doubles(L) * sizeof(double), ctx->stream, c, L, P.d_pd,
                     P.d_tab, bessel_order == 0 ? ctx->d_j0 : ctx->d_j2, nullptr, nullptr);
  hipLaunchKernelGGL(k_proj_kernel_spline, dim3(1), dim3(64),
                     (size_t)(11 * L.NKT) * sizeof(double), ctx->stream, L, P.d_tab);
  HIPCHK(hipGetLastError());
  P.ready = true;
  P.me_ready = true;
  side.end();                      // (marks the projection set-up as pending)
  return CHOMP_OK;
}

int chomp_multi_epoch_setup(chomp_ctx* ctx, const chomp_cosmo* cosmo, double z_min,
                            double z_max) {
  if (!ctx || !cosmo) return fail(ctx, CHOMP_ERR_ARG, "multi_epoch_setup: bad args");
  if (!ctx->dark_energy && has_dark_energy(cosmo->w0, cosmo->wa))
    return fail(ctx, CHOMP_ERR_SCOPE, "multi_epoch_setup: w0/wa != -1/0 needs chomp_set_dark_energy(ctx, 1)");
  if (!(z_max > z_min)) return fail(ctx, CHOMP_ERR_ARG, "multi_epoch_setup: z range");
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  SideScope side(ctx, &ctx->ev_proj_ready, true);
  { const int rcs = side.begin(); if (rcs) return rcs; }
  const chomp_config& c = ctx->cfg;
  ProjState& P = ctx->proj;
  P.ready = false;
  P.me_ready = false;
  P.cov_ready = false;
  P.ssc_ready = false;
  P.ssc_prep = false;
  P.ng_ready = false;
  P.ng_prep = false;
  P.L = make_proj_layout(c.cosmo_npoints, c.window_npoints, c.kernel_npoints);
  HIPCHK((hipError_t)P.d_pd.once(1));
  HIPCHK((hipError_t)P.d_pd_init.once(1));
  { const int rce = ensure(ctx, P.d_tab, (size_t)P.L.total); if (rce) return rce; }
  ProjDev pd;
  std::memset(&pd, 0, sizeof(pd));
  pd.om0 = cosmo->omega_m0; pd.ol0 = cosmo->omega_l0; pd.or0 = cosmo->omega_r0;
  pd.H0 = 100.0 / (2.998 * 100000.0);
  pd.growth_norm = growth_approx(pd.om0, pd.ol0, 1.0);
  pd.me_z_min[0] = z_min < 0.0 ? 0.0 : z_min;
  pd.me_z_max[0] = z_max;
  { const int rcp = upload(ctx, P.d_pd_init, &pd, sizeof(pd), ctx->sh_proj); if (rcp) return rcp; }
  HIPCHK(hipMemcpyAsync(P.d_pd, P.d_pd_init, sizeof(pd), hipMemcpyDeviceToDevice, ctx->stream));
  if (P.L.NC > 240) return fail(ctx, CHOMP_ERR_ARG, "multi_epoch_setup: cosmo_npoints too large");
  DeSpline de;
  { const int rcd = proj_dark_energy(ctx, cosmo, &de); if (rcd) return rcd; }
  if (P.de)
    hipLaunchKernelGGL(k_proj_chi<true>, dim3(P.L.NC, 1), dim3(64), 0, ctx->stream, c, P.L, P.d_pd, P.d_tab, de);
  else
    hipLaunchKernelGGL(k_proj_chi<false>, dim3(P.L.NC, 1), dim3(64), 0, ctx->stream, c, P.L, P.d_pd, P.d_tab, de);
  hipLaunchKernelGGL(k_proj_me_splines, dim3(1), dim3(192),
                     (size_t)(33 * P.L.NC) * sizeof(double), ctx->stream, c, P.L, P.d_pd, P.d_tab);
  HIPCHK(hipGetLastError());
  P.me_ready = true;
  side.end();                      // (marks the projection set-up as pending)
  return CHOMP_OK;
}

int chomp_me_eval(chomp_ctx* ctx, int what, const double* x, size_t n, double* out, int mem) {
  if (!ctx || !x || !out || n == 0 || what < 0 || what > 2) return fail(ctx, CHOMP_ERR_ARG, "me_eval: bad args");
  Staging st(ctx, mem, "me_eval");
  if (st.rc) return st.rc;
  if (!ctx->proj.me_ready) return fail(ctx, CHOMP_ERR_STATE, "me_eval before multi_epoch_setup / kernel_setup");
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  const double* din;
  double* dout;
  st.in(x, n, &din);
  st.out(out, n, &dout);
  const int rc = st.place();
  if (rc) return rc;
  hipLaunchKernelGGL(k_me_eval, grid_1d(n), dim3(256), 0, ctx->stream, ctx->proj.L,
                     ctx->proj.d_pd, ctx->proj.d_tab, what, din, (int)n, dout);
  return st.finish();
}

// The CHOMP_KI_* scalars of one set-up's block.
static void proj_info_out(const ProjDev& pd, double* out) {
  out[CHOMP_KI_Z_BAR] = pd.z_bar; out[CHOMP_KI_CHI_MIN] = pd.chi_min;
  out[CHOMP_KI_CHI_MAX] = pd.chi_max; out[CHOMP_KI_Z_MIN] = pd.z_min;
  out[CHOMP_KI_Z_MAX] = pd.z_max; out[CHOMP_KI_D_ZBAR] = pd.D_zbar;
  out[CHOMP_KI_NORM_A] = pd.dist[0].norm; out[CHOMP_KI_NORM_B] = pd.dist[1].norm;
  out[CHOMP_KI_WA_CHI_MIN] = pd.w_chi_min[0]; out[CHOMP_KI_WA_CHI_MAX] = pd.w_chi_max[0];
  out[CHOMP_KI_WB_CHI_MIN] = pd.w_chi_min[1]; out[CHOMP_KI_WB_CHI_MAX] = pd.w_chi_max[1];
  out[CHOMP_KI_J_LIMIT] = pd.j_limit;
}

// Where table CHOMP_KTAB_* lies in a slab of the layout; false: no such table.
static bool proj_table_span(const ProjLayout& L, int table, int* off, size_t* len) {
  switch (table) {
    case CHOMP_KTAB_LN_KTHETA: *off = L.k_ln; *len = L.NKT; break;
    case CHOMP_KTAB_KERNEL: *off = L.k_arr; *len = L.NKT; break;
    case CHOMP_KTAB_LEVELS: *off = L.k_lev; *len = L.NKT; break;
    case CHOMP_KTAB_WA_CHI: *off = L.w_chi[0]; *len = L.NWp; break;
    case CHOMP_KTAB_WA: *off = L.w_wf[0]; *len = L.NWp; break;
    case CHOMP_KTAB_WB_CHI: *off = L.w_chi[1]; *len = L.NWp; break;
    case CHOMP_KTAB_WB: *off = L.w_wf[1]; *len = L.NWp; break;
    case CHOMP_KTAB_ME_Z: *off = L.me_z[0]; *len = L.NC; break;
    case CHOMP_KTAB_ME_CHI: *off = L.me_chi[0]; *len = L.NC; break;
    case CHOMP_KTAB_ME_GROWTH: *off = L.me_growth[0]; *len = L.NC; break;
    default: return false;
  }
  return true;
}

int chomp_kernel_info(chomp_ctx* ctx, double* out) {
  if (!ctx || !out) return fail(ctx, CHOMP_ERR_ARG, "kernel_info: bad args");
  if (!ctx->proj.ready) return fail(ctx, CHOMP_ERR_STATE, "kernel_info before kernel_setup");
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ProjDev& pd = ctx->proj.host;
  HIPCHK(hipMemcpy(&pd, ctx->proj.d_pd, sizeof(pd), hipMemcpyDeviceToHost));
  proj_info_out(pd, out);
  return CHOMP_OK;
}

int chomp_kernel_table(chomp_ctx* ctx, int table, double* out, size_t n) {
  if (!ctx || !out) return fail(ctx, CHOMP_ERR_ARG, "kernel_table: bad args");
  if (!ctx->proj.me_ready) return fail(ctx, CHOMP_ERR_STATE, "kernel_table before kernel_setup");
  if (!ctx->proj.ready && table != CHOMP_KTAB_ME_Z && table != CHOMP_KTAB_ME_CHI &&
      table != CHOMP_KTAB_ME_GROWTH)
    return fail(ctx, CHOMP_ERR_STATE, "kernel_table: only the MultiEpoch tables exist");
  int off = -1;
  size_t len = 0;
  if (!proj_table_span(ctx->proj.L, table, &off, &len)) return fail(ctx, CHOMP_ERR_ARG, "kernel_table: unknown table");
  if (n != len) return fail(ctx, CHOMP_ERR_ARG, "kernel_table: length mismatch");
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(out, ctx->proj.d_tab + off, len * sizeof(double), hipMemcpyDeviceToHost));
  return CHOMP_OK;
}

// n_set projection set-ups on the set axis (chomp_proj_kernels.h, "The set axis"): the six launches
// of chomp_kernel_setup, once, with the set as the grids' z dimension.  Set s takes cosmo[s],
// me_z_min[s * step], me_z_max[s * step], a[s * step] and b[s * step] (step 0: one range and one
// window pair for every set; 1: arrays); the k theta range and the Bessel order are shared.  The
// callers have validated their arguments.  On the context's stream; ctx->proj is not touched.
// Tabulated redshift distributions go to the sets' arena (chomp_pp_plan.h: equal tables share a
// place) ahead of the launches; with a w0-wa cosmology among the sets, the distinct (w0, wa) get
// their pressure tables in S.de and the two kernels that evaluate E(z) run their <true> forms.
// who: the caller's name.
static int kernel_sets_launch(chomp_ctx* ctx, const char* who, size_t n_set, const chomp_cosmo* cosmo,
                              const double* me_z_min, const double* me_z_max, size_t step,
                              double ktheta_min, double ktheta_max, const chomp_window* a,
                              const chomp_window* b, int bessel_order) {
  const std::string w_ = std::string(who) + ": ";
  const chomp_config& c = ctx->cfg;
  const ProjLayout L = make_proj_layout(c.cosmo_npoints, c.window_npoints, c.kernel_npoints);
  if (L.NC > 240 || L.NWp > 360 || L.NKT > 720)          // (the spline builds are staged in 64 KB of LDS)
    return fail(ctx, CHOMP_ERR_ARG, w_ + "cosmo/window/kernel_npoints too large");
  HIPCHK(hipSetDevice(ctx->device));
  ProjSets& S = ctx->sets;
  S.n = 0;
  int rc = ensure(ctx, S.d_pd, n_set);
  if (!rc) rc = ensure(ctx, S.d_pd_init, n_set);
  if (!rc) rc = ensure(ctx, S.d_tab, n_set * (size_t)L.total);
  if (rc) return rc;
  // the tables of the windows (step 0: of the one pair), window w of set s at [2 s + w]
  const size_t n_pair = step ? n_set : 1;
  std::vector<PpTable> tables(2 * n_pair, PpTable{nullptr, nullptr, 0, 0});
  bool tabulated = false;
  for (size_t s = 0; s < n_pair; ++s)
    for (int w = 0; w < 2; ++w) {
      const chomp_dndz& dz = (w == 0 ? a : b)[s].dist;
      if (dz.kind != CHOMP_DNDZ_PPOLY) continue;
      tables[2 * s + w] = PpTable{dz.pp_breaks, dz.pp_coef, dz.pp_n, dz.pp_order};
      tabulated = true;
    }
  PpPlan plan;
  if (tabulated) {
    if (!pp_plan(tables.data(), tables.size(), &plan))
      return fail(ctx, CHOMP_ERR_ARG, w_ + "the distinct tabulated redshift distributions of one call "
                                           "exceed " + std::to_string(kPpArenaMax) + " doubles");
    rc = ensure(ctx, S.d_pp, plan.total);
    if (rc) return rc;
    std::vector<double> arena(plan.total);
    pp_pack(tables.data(), plan, arena.data());
    rc = upload(ctx, S.d_pp, arena.data(), plan.total * sizeof(double));
    if (rc) return rc;
  }
  // the pressure tables of the distinct (w0, wa), and every set's
  std::vector<DePar> de_keys;
  std::vector<int> de_slot(n_set, -1);
  for (size_t s = 0; s < n_set; ++s) {
    if (!has_dark_energy(cosmo[s].w0, cosmo[s].wa)) continue;
    size_t q = 0;
    while (q < de_keys.size() && !(de_keys[q].w0 == cosmo[s].w0 && de_keys[q].wa == cosmo[s].wa)) ++q;
    if (q == de_keys.size()) de_keys.push_back(DePar{cosmo[s].w0, cosmo[s].wa});
    de_slot[s] = (int)q;
  }
  DeSets de{nullptr, nullptr, 0, 0};
  if (!de_keys.empty()) {
    rc = de_build(ctx, S.de, de_keys);
    if (!rc) rc = ensure(ctx, S.d_de_slot, n_set);
    if (!rc) rc = upload(ctx, S.d_de_slot, de_slot.data(), n_set * sizeof(int));
    if (rc) return rc;
    de = DeSets{S.de.d_tab, S.d_de_slot, de_stride(c.cosmo_npoints), c.cosmo_npoints};
  }
  const double j_limit = bessel_zero_host(bessel_order, c.kernel_bessel_limit);
  std::vector<ProjDev> pd(n_set);
  for (size_t s = 0; s < n_set; ++s) {
    const chomp_window* ws[2] = {&a[s * step], &b[s * step]};
    pd[s] = proj_host_block(c, &cosmo[s], me_z_min[s * step], me_z_max[s * step], ktheta_min,
                            ktheta_max, ws, bessel_order, j_limit);
    for (int w = 0; w < 2 && tabulated; ++w) {
      const long long at = plan.offset[2 * (s * step) + w];
      if (at < 0) continue;
      pd[s].dist[w].pp = S.d_pp + at;
      pd[s].dist[w].pp_n = ws[w]->dist.pp_n;
      pd[s].dist[w].pp_order = ws[w]->dist.pp_order;
    }
  }
  rc = upload(ctx, S.d_pd_init, pd.data(), n_set * sizeof(ProjDev));
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(S.d_pd, S.d_pd_init, n_set * sizeof(ProjDev), hipMemcpyDeviceToDevice, ctx->stream));
  S.L = L;
  S.host = pd[0];                   // (what the sets share: the ln k theta range and the order)
  ctx->sets_z_min.resize(n_set);    // kernel.py:910-916, each set's share (as CrossState::z_min / z_max)
  ctx->sets_z_max.resize(n_set);
  for (size_t s = 0; s < n_set; ++s) {
    ctx->sets_z_min[s] = std::max(pd[s].w_z_min[0], pd[s].w_z_min[1]);
    ctx->sets_z_max[s] = std::min(pd[s].w_z_max[0], pd[s].w_z_max[1]);
  }
  const unsigned Z = (unsigned)n_set;
  const size_t stride = (size_t)L.total;
  if (de.tab)
    hipLaunchKernelGGL(k_proj_chi_sets<true>, dim3(L.NC, 4, Z), dim3(64), 0, ctx->stream, c, L, S.d_pd, S.d_tab, stride, de);
  else
    hipLaunchKernelGGL(k_proj_chi_sets<false>, dim3(L.NC, 4, Z), dim3(64), 0, ctx->stream, c, L, S.d_pd, S.d_tab, stride, de);
  hipLaunchKernelGGL(k_proj_me_splines_sets, dim3(3, 1, Z), dim3(192), (size_t)(33 * L.NC) * sizeof(double),
                     ctx->stream, c, L, S.d_pd, S.d_tab, stride);
  if (de.tab)
    hipLaunchKernelGGL(k_proj_window_sets<true>, dim3(L.NWp, 2, Z), dim3(64),
                       (size_t)(L.NC + 4 * (L.NC - 1)) * sizeof(double), ctx->stream, c, L, S.d_pd,
                       S.d_tab, stride, de);
  else
    hipLaunchKernelGGL(k_proj_window_sets<false>, dim3(L.NWp, 2, Z), dim3(64),
                       (size_t)(L.NC + 4 * (L.NC - 1)) * sizeof(double), ctx->stream, c, L, S.d_pd,
                       S.d_tab, stride, de);
  hipLaunchKernelGGL(k_proj_window_splines_sets, dim3(1, 1, Z), dim3(128),
                     (size_t)(22 * L.NWp) * sizeof(double), ctx->stream, c, L, S.d_pd, S.d_tab, stride);
  hipLaunchKernelGGL(k_proj_kernel_knots_sets, dim3(L.NKT, 1, Z), dim3(256),
                     (size_t)ProjLds::doubles(L) * sizeof(double), ctx->stream, c, L, S.d_pd,
                     S.d_tab, bessel_order == 0 ? ctx->d_j0 : ctx->d_j2, stride);
  hipLaunchKernelGGL(k_proj_kernel_spline_sets, dim3(1, 1, Z), dim3(64),
                     (size_t)(11 * L.NKT) * sizeof(double), ctx->stream, L, S.d_tab, stride);
  HIPCHK(hipGetLastError());
  S.n = n_set;
  return CHOMP_OK;
}

// One projection set-up per cosmology (the cosmology axis of a w(theta) design or chain:
// Kernel.set_cosmology, kernel.py:657-676, once per point of simulation_design.py:116-155):
// kernel_sets_launch with the range and the windows of every set the same.
int chomp_kernel_setup_sets(chomp_ctx* ctx, size_t n_set, const chomp_cosmo* cosmo, double me_z_min,
                            double me_z_max, double ktheta_min, double ktheta_max,
                            const chomp_window* a, const chomp_window* b, int bessel_order) {
  StageRange range_(ctx, "chomp:kernel_setup_sets");
  if (!ctx || !cosmo || !a || !b || n_set == 0) return fail(ctx, CHOMP_ERR_ARG, "kernel_setup_sets: bad args");
  if (n_set > (size_t)kProjSetsMax)
    return fail(ctx, CHOMP_ERR_ARG, "kernel_setup_sets: more than " + std::to_string(kProjSetsMax) + " sets in one call");
  if (bessel_order != 0 && bessel_order != 2) return fail(ctx, CHOMP_ERR_ARG, "kernel_setup_sets: bessel order must be 0 or 2");
  for (size_t s = 0; s < n_set && !(ctx->sets_scope & CHOMP_SETS_DARK_ENERGY); ++s)
    if (has_dark_energy(cosmo[s].w0, cosmo[s].wa))
      return fail(ctx, CHOMP_ERR_SCOPE, "kernel_setup_sets: a w0/wa != -1/0 cosmology is set up by chomp_kernel_setup");
  const chomp_window* ws[2] = {a, b};
  { const int rcc = proj_check_args(ctx, "kernel_setup_sets", ktheta_min, ktheta_max, ws); if (rcc) return rcc; }
  for (int w = 0; w < 2 && !(ctx->sets_scope & CHOMP_SETS_TABULATED); ++w)
    if (ws[w]->dist.kind == CHOMP_DNDZ_PPOLY)
      return fail(ctx, CHOMP_ERR_SCOPE, "kernel_setup_sets: a tabulated redshift distribution "
                                        "(dNdzInterpolation) is set up by chomp_kernel_setup");
  return kernel_sets_launch(ctx, "kernel_setup_sets", n_set, cosmo, &me_z_min, &me_z_max, 0, ktheta_min,
                            ktheta_max, a, b, bessel_order);
}

// One projection set-up per kernel (the window pairs of a tomographic analysis, each with its
// own MultiEpoch range and cosmology: a Kernel / GalaxyGalaxyLensingKernel per set, kernel.py:
// 559-839), on the same set axis: chomp_kernel_info_sets, chomp_kernel_table_set, chomp_wtheta_sets
// and chomp_cell_sets serve either set-up.  Every set is validated before anything is launched,
// and a refusal names the set.
int chomp_kernel_setup_pairs(chomp_ctx* ctx, size_t n_set, const chomp_cosmo* cosmo,
                             const double* me_z_min, const double* me_z_max, double ktheta_min,
                             double ktheta_max, const chomp_window* a, const chomp_window* b,
                             int bessel_order) {
  StageRange range_(ctx, "chomp:kernel_setup_pairs");
  if (!ctx || !cosmo || !me_z_min || !me_z_max || !a || !b || n_set == 0)
    return fail(ctx, CHOMP_ERR_ARG, "kernel_setup_pairs: bad args");
  if (n_set > (size_t)kProjSetsMax)
    return fail(ctx, CHOMP_ERR_ARG, "kernel_setup_pairs: more than " + std::to_string(kProjSetsMax) + " sets in one call");
  if (bessel_order != 0 && bessel_order != 2) return fail(ctx, CHOMP_ERR_ARG, "kernel_setup_pairs: bessel order must be 0 or 2");
  for (size_t s = 0; s < n_set; ++s) {
    const std::string ws_ = "kernel_setup_pairs: set " + std::to_string(s);
    if (!(ctx->sets_scope & CHOMP_SETS_DARK_ENERGY) && has_dark_energy(cosmo[s].w0, cosmo[s].wa))
      return fail(ctx, CHOMP_ERR_SCOPE, ws_ + ": a w0/wa != -1/0 cosmology is set up by chomp_kernel_setup");
    const chomp_window* ws[2] = {&a[s], &b[s]};
    { const int rcc = proj_check_args(ctx, ws_.c_str(), ktheta_min, ktheta_max, ws); if (rcc) return rcc; }
    for (int w = 0; w < 2 && !(ctx->sets_scope & CHOMP_SETS_TABULATED); ++w)
      if (ws[w]->dist.kind == CHOMP_DNDZ_PPOLY)
        return fail(ctx, CHOMP_ERR_SCOPE, ws_ + ": a tabulated redshift distribution "
                                          "(dNdzInterpolation) is set up by chomp_kernel_setup");
  }
  return kernel_sets_launch(ctx, "kernel_setup_pairs", n_set, cosmo, me_z_min, me_z_max, 1, ktheta_min,
                            ktheta_max, a, b, bessel_order);
}

// chomp_kernel_info of every set, [n_set][CHOMP_KI_COUNT], in one synchronising read-back.
int chomp_kernel_info_sets(chomp_ctx* ctx, double* out) {
  if (!ctx || !out) return fail(ctx, CHOMP_ERR_ARG, "kernel_info_sets: bad args");
  const ProjSets& S = ctx->sets;
  if (S.n == 0) return fail(ctx, CHOMP_ERR_STATE, "kernel_info_sets before kernel_setup_sets / kernel_setup_pairs");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::vector<ProjDev> pd(S.n);
  HIPCHK(hipMemcpy(pd.data(), S.d_pd, S.n * sizeof(ProjDev), hipMemcpyDeviceToHost));
  for (size_t s = 0; s < S.n; ++s) proj_info_out(pd[s], out + s * CHOMP_KI_COUNT);
  return CHOMP_OK;
}

// chomp_kernel_table of one set.
int chomp_kernel_table_set(chomp_ctx* ctx, size_t set, int table, double* out, size_t n) {
  if (!ctx || !out) return fail(ctx, CHOMP_ERR_ARG, "kernel_table_set: bad args");
  const ProjSets& S = ctx->sets;
  if (S.n == 0) return fail(ctx, CHOMP_ERR_STATE, "kernel_table_set before kernel_setup_sets / kernel_setup_pairs");
  if (set >= S.n) return fail(ctx, CHOMP_ERR_ARG, "kernel_table_set: set");
  int off = -1;
  size_t len = 0;
  if (!proj_table_span(S.L, table, &off, &len)) return fail(ctx, CHOMP_ERR_ARG, "kernel_table_set: unknown table");
  if (n != len) return fail(ctx, CHOMP_ERR_ARG, "kernel_table_set: length mismatch");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(out, S.d_tab + set * (size_t)S.L.total + off, len * sizeof(double), hipMemcpyDeviceToHost));
  return CHOMP_OK;
}

int chomp_kernel_raw(chomp_ctx* ctx, const double* ln_ktheta, size_t n, double* out, int mem) {
  if (!ctx || !ln_ktheta || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "kernel_raw: bad args");
  Staging st(ctx, mem, "kernel_raw");
  if (st.rc) return st.rc;
  if (!ctx->proj.ready) return fail(ctx, CHOMP_ERR_STATE, "kernel_raw before kernel_setup");
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  const double* din;
  double* dout;
  st.in(ln_ktheta, n, &din);
  st.out(out, n, &dout);
  const int rc = st.place();
  if (rc) return rc;
  const ProjLayout& L = ctx->proj.L;
  hipLaunchKernelGGL(k_proj_kernel_knots, dim3((unsigned)n), dim3(256),
                     (size_t)ProjLds::doubles(L) * sizeof(double), ctx->stream, ctx->cfg, L,
                     ctx->proj.d_pd, ctx->proj.d_tab,
                     ctx->proj.host.order == 0 ? ctx->d_j0 : ctx->d_j2, din, dout);
  return st.finish();
}

int chomp_kernel_eval(chomp_ctx* ctx, const double* x, size_t n, double* out, int mem) {
  if (!ctx || !x || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "kernel_eval: bad args");
  Staging st(ctx, mem, "kernel_eval");
  if (st.rc) return st.rc;
  if (!ctx->proj.ready) return fail(ctx, CHOMP_ERR_STATE, "kernel_eval before kernel_setup");
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  const double* din;
  double* dout;
  st.in(x, n, &din);
  st.out(out, n, &dout);
  const int rc = st.place();
  if (rc) return rc;
  hipLaunchKernelGGL(k_kernel_eval, grid_1d(n), dim3(256), 0, ctx->stream, ctx->proj.L,
                     ctx->proj.d_pd, ctx->proj.d_tab, din, (int)n, dout);
  return st.finish();
}

int chomp_window_eval(chomp_ctx* ctx, int which, const double* x, size_t n, double* out, int mem) {
  if (!ctx || !x || !out || n == 0 || which < 0 || which > 1) return fail(ctx, CHOMP_ERR_ARG, "window_eval: bad args");
  Staging st(ctx, mem, "window_eval");
  if (st.rc) return st.rc;
  if (!ctx->proj.ready) return fail(ctx, CHOMP_ERR_STATE, "window_eval before kernel_setup");
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  const double* din;
  double* dout;
  st.in(x, n, &din);
  st.out(out, n, &dout);
  const int rc = st.place();
  if (rc) return rc;
  hipLaunchKernelGGL(k_window_eval, grid_1d(n), dim3(256), 0, ctx->stream, ctx->proj.L,
                     ctx->proj.d_pd, ctx->proj.d_tab, which, din, (int)n, dout);
  return st.finish();
}

static int wtheta_impl(chomp_ctx* ctx, int which, size_t epoch, double k_min, double k_max, double D_z,
                       const double* theta, size_t n, double* out, int mem) {
  if (!ctx || !theta || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "wtheta: bad args");
  Staging st(ctx, mem, "wtheta");
  if (st.rc) return st.rc;
  if (!ctx->proj.ready) return fail(ctx, CHOMP_ERR_STATE, "wtheta before kernel_setup");
  int rc = check_power(ctx, which, epoch, 1);
  if (rc) return rc;
  if (ctx->with_bao && ctx->precision != CHOMP_PREC_F64)
    return fail(ctx, CHOMP_ERR_SCOPE, "wtheta: the narrowed precision modes exist for the no-wiggle spectrum only");
  if (!(k_min > 0.0) || !(k_max > k_min) || !(D_z > 0.0)) return fail(ctx, CHOMP_ERR_ARG, "wtheta: k range / D_z");
  HIPCHK(hipSetDevice(ctx->device));
  rc = prepare_extrapolation(ctx, which, epoch, 1);
  if (rc) return rc;
  const double* din;
  double* dout;
  st.in(theta, n, &din);
  st.out(out, n, &dout);
  rc = st.place();
  if (rc) return rc;
  const ProjLayout& L = ctx->proj.L;
  const WthPlan P = wth_plan(ctx->cfg.divmax, ctx->L.NK, L, ctx->proj.host.ln_kt_min,
                             ctx->proj.host.ln_kt_max, k_min, k_max, ctx->tune[CHOMP_TUNE_WTHETA_DIRECT]);
  const int LT = P.LT, nseg = P.nseg;
  if (ctx->precision != CHOMP_PREC_F64) {
    auto mixed = [&](auto PREC) {
      hipLaunchKernelGGL(k_wtheta_mixed<PREC>, dim3((unsigned)n), dim3(256), P.sh, ctx->stream, ctx->cfg,
                         ctx->L, L, ctx->d_epochs, (int)epoch, ctx->d_tab, which, ctx->proj.d_pd,
                         ctx->proj.d_tab, k_min, k_max, D_z, din, dout);
    };
    switch (ctx->precision) {
      case CHOMP_PREC_F32_EVAL: mixed(int_c<CHOMP_PREC_F32_EVAL>{}); break;
      case CHOMP_PREC_F32_TABLES: mixed(int_c<CHOMP_PREC_F32_TABLES>{}); break;
      default: mixed(int_c<CHOMP_PREC_F32_ALL>{}); break;
    }
    return st.finish();
  }
  // fp64: the theta-independent factor of the integrand on the Romberg nodes first, then the
  // moment route (k_wtheta_moments + k_wtheta_fast) or k_wtheta, as the plan says (WthPlan: the
  // node table, then the moment records and the segments' totals -- one epoch's scratch)
  rc = ensure(ctx, ctx->d_wnodes, P.stride);
  if (rc) return rc;
  double* rec = ctx->d_wnodes + P.rec_at;
  double* segtot = ctx->d_wnodes + P.tot_at;
  with_flag(which & CHOMP_P_HALOFIT, ctx->with_bao, [&](auto HF, auto BAO) {
    hipLaunchKernelGGL((k_wtheta_nodes<HF, BAO>), dim3(P.gnodes), dim3(256), P.sh_nodes, ctx->stream,
                       ctx->cfg, ctx->L, ctx->d_epochs, (int)epoch, ctx->d_tab, which, k_min, k_max,
                       D_z, LT, ctx->d_wnodes);
    if (P.fast) {
      hipLaunchKernelGGL(k_wtheta_moments, dim3((unsigned)nseg, (unsigned)LT, kWthParts), dim3(256), 0,
                         ctx->stream, ctx->d_wnodes, LT, nseg, std::log(k_min), std::log(k_max), rec,
                         segtot);
      hipLaunchKernelGGL(k_wtheta_fast, dim3((unsigned)n), dim3(256), 0, ctx->stream, ctx->cfg, L,
                         ctx->proj.d_pd, ctx->proj.d_tab, k_min, k_max, din, dout, ctx->d_wnodes, rec,
                         segtot, LT, nseg);
    } else {
      hipLaunchKernelGGL((k_wtheta<HF, BAO>), dim3((unsigned)n), dim3(64 * kWthetaNW), P.sh, ctx->stream,
                         ctx->cfg, ctx->L, L, ctx->d_epochs, (int)epoch, ctx->d_tab, which, ctx->proj.d_pd,
                         ctx->proj.d_tab, k_min, k_max, D_z, din, dout, ctx->d_wnodes, LT);
    }
  });
  return st.finish();
}

int chomp_xi3d(chomp_ctx* ctx, int which, size_t epoch, double k_min, double k_max,
               const double* r, size_t n, double* out, int mem) {
  if (!ctx || !r || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "xi3d: bad args");
  Staging st(ctx, mem, "xi3d");
  if (st.rc) return st.rc;
  int rc = check_power(ctx, which, epoch, 1);
  if (rc) return rc;
  if (!(k_min > 0.0) || !(k_max > k_min)) return fail(ctx, CHOMP_ERR_ARG, "xi3d: k range");
  HIPCHK(hipSetDevice(ctx->device));
  rc = prepare_extrapolation(ctx, which, epoch, 1);
  if (rc) return rc;
  const double* din;
  double* dout;
  st.in(r, n, &din);
  st.out(out, n, &dout);
  rc = st.place();
  if (rc) return rc;
  const size_t sh = (size_t)(12 * (ctx->L.NK - 1)) * sizeof(double);
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_xi3d<BAO>, dim3((unsigned)n), dim3(256), sh, ctx->stream, ctx->cfg,
                       ctx->L, ctx->d_epochs, (int)epoch, ctx->d_tab, which, ctx->d_j0, k_min,
                       k_max, din, dout);
  });
  return st.finish();
}

// -- the batched calls: w(theta), xi(r) and C_l of many epochs ---------------------------------
// What they share is written once: the plans of the scratch and the launches (WthPlan, CellPlan:
// chomp_proj_kernels.h), the chunk rule, the refusals, and per observable one chunked driver
// (wtheta_rows, cell_rows).  In messages a call names itself (`who`) and the single-epoch call
// that serves what it does not (`single`).

// The epochs of one chunk: kWthEpochChunk unless CHOMP_TUNE_WTHETA_EPOCH_CHUNK says otherwise.
static size_t epoch_chunk(const chomp_ctx* ctx, size_t n_epoch) {
  const long long tuned = ctx->tune[CHOMP_TUNE_WTHETA_EPOCH_CHUNK];
  const size_t chunk = tuned > 0 ? (size_t)tuned : (size_t)kWthEpochChunk;
  return std::min(std::min(chunk, (size_t)kWthEpochChunkMax), n_epoch);
}

// arrays: every array argument is there
static int batch_args(chomp_ctx* ctx, const char* who, bool arrays, size_t n, size_t n_epoch) {
  if (!arrays || n == 0 || n_epoch == 0) return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": bad args");
  if (n > 0x7fffffffu / n_epoch) return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": n * n_epoch too large");
  return CHOMP_OK;
}

// What the batched calls do not serve is said before the spectrum is looked at: a HaloFit code on
// epochs without a HaloFit set-up is out of scope here, not a state to repair.  fp64_note: why,
// where the single call has no narrowed precision mode either.
static int batch_scope(chomp_ctx* ctx, const char* who, const char* single, int which,
                       const char* fp64_note = nullptr) {
  if (ctx->precision != CHOMP_PREC_F64) {
    const std::string why = fp64_note ? fp64_note : std::string("the narrowed precision modes belong to ") + single;
    return fail(ctx, CHOMP_ERR_SCOPE, std::string(who) + ": fp64 only (" + why + ")");
  }
  const char* what = nullptr;
  if (which & CHOMP_P_HALOFIT) what = ": HaloFit spectra are";
  else if ((which & CHOMP_P_EXTRAPOLATE) && (which & 15) != CHOMP_P_LIN) what = ": extrapolated spectra are";
  else if (ctx->with_bao) what = ": the wiggle transfer function is";
  if (!what) return CHOMP_OK;
  return fail(ctx, CHOMP_ERR_SCOPE, std::string(who) + what + " evaluated by " + single);
}

// xi(r) of n_epoch epochs that share the k range (an HOD or cosmology design or chain): the node
// table of chomp_wtheta_epochs with D_z = 1.0 -- the r-independent factor of the integrand, once
// per epoch -- and one Romberg launch with an epoch axis that reads it, the epochs worked off in
// chunks (layout: chomp_proj_kernels.h, k_xi3d_epochs).  No projection set-up.
int chomp_xi3d_epochs(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, double k_min,
                      double k_max, const double* r, size_t n, double* out, int mem) {
  StageRange range_(ctx, "chomp:xi3d_epochs");
  if (!ctx) return CHOMP_ERR_ARG;
  int rc = batch_args(ctx, "xi3d_epochs", r && out, n, n_epoch);
  if (rc) return rc;
  Staging st(ctx, mem, "xi3d_epochs");
  if (st.rc) return st.rc;
  rc = batch_scope(ctx, "xi3d_epochs", "chomp_xi3d", which);
  if (rc) return rc;
  if (ctx->cfg.divmax > kWthetaTabLevel)
    return fail(ctx, CHOMP_ERR_SCOPE, "xi3d_epochs: divmax beyond the node table (level 20) is evaluated by chomp_xi3d");
  rc = check_power(ctx, which, epoch0, n_epoch);
  if (rc) return rc;
  if (!(k_min > 0.0) || !(k_max > k_min)) return fail(ctx, CHOMP_ERR_ARG, "xi3d_epochs: k range");
  HIPCHK(hipSetDevice(ctx->device));
  const double* din;
  double* dout;
  st.in(r, n, &din);
  st.out(out, n * n_epoch, &dout);
  rc = st.place();
  if (rc) return rc;
  // (the node-table part of the w(theta) plan: every level, divmax <= kWthetaTabLevel)
  const WthPlan P = wth_plan_of(ctx->cfg.divmax, 1, false, ctx->L.NK);
  const size_t chunk = epoch_chunk(ctx, n_epoch);
  rc = ensure(ctx, ctx->d_wnodes, P.stride * chunk);
  if (rc) return rc;
  for (size_t c0 = 0; c0 < n_epoch; c0 += chunk) {          // (the scratch is reused in stream order)
    const unsigned E = (unsigned)std::min(chunk, n_epoch - c0);
    hipLaunchKernelGGL((k_wtheta_nodes_epochs<false, false>), dim3(P.gnodes, E), dim3(256), P.sh_nodes,
                       ctx->stream, ctx->cfg, ctx->L, ctx->d_epochs, (int)(epoch0 + c0), ctx->d_tab,
                       which, k_min, k_max, 1.0, P.LT, ctx->d_wnodes, P.stride);
    hipLaunchKernelGGL(k_xi3d_epochs, dim3((unsigned)n, E), dim3(256), 0, ctx->stream,
                       ctx->cfg.global_precision, ctx->cfg.corr_precision, ctx->cfg.divmax,
                       ctx->d_j0, k_min, k_max, din, dout + c0 * n, ctx->d_wnodes, P.stride);
  }
  return st.finish();
}

int chomp_spline_eval(chomp_ctx* ctx, const double* xk, const double* yk, size_t nk,
                      const double* x, size_t n, int deriv, double* out) {
  if (!ctx || !xk || !yk || !x || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "spline_eval: bad args");
  if (nk < 4 || nk > 4096) return fail(ctx, CHOMP_ERR_ARG, "spline_eval: 4 <= nk <= 4096");
  if (deriv != 0 && deriv != 1) return fail(ctx, CHOMP_ERR_ARG, "spline_eval: deriv must be 0 or 1");
  for (size_t i = 1; i < nk; ++i)
    if (!(xk[i] > xk[i - 1])) return fail(ctx, CHOMP_ERR_ARG, "spline_eval: knots must increase");
  HIPCHK(hipSetDevice(ctx->device));
  Staging st(ctx, CHOMP_HOST, "spline_eval");
  const double *d_xk, *d_yk, *dx;
  double* dout;
  st.in(xk, nk, &d_xk);
  st.in(yk, nk, &d_yk);
  st.in(x, n, &dx);
  st.out(out, n, &dout);
  const int rc = st.place(4 * (nk - 1) + 2 * nk);   // scratch: the coefficients, then work
  if (rc) return rc;
  hipLaunchKernelGGL(k_spline_eval, dim3(1), dim3(256), 0, ctx->stream, d_xk, d_yk, (int)nk,
                     st.scratch, st.scratch + 4 * (nk - 1), dx, (int)n, deriv, dout);
  return st.finish();
}

int chomp_set_precision(chomp_ctx* ctx, int mode) {
  if (!ctx) return CHOMP_ERR_ARG;
  if (mode < CHOMP_PREC_F64 || mode > CHOMP_PREC_F32_ALL)
    return fail(ctx, CHOMP_ERR_ARG, "set_precision: unknown mode");
  ctx->precision = mode;
  return CHOMP_OK;
}

static int cell_impl(chomp_ctx* ctx, int which, size_t epoch, double D_z, const double* ell, size_t n,
                     double* out, int mem) {
  if (!ctx || !ell || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "cell: bad args");
  Staging st(ctx, mem, "cell");
  if (st.rc) return st.rc;
  if (!ctx->proj.ready) return fail(ctx, CHOMP_ERR_STATE, "cell before kernel_setup");
  int rc = check_power(ctx, which, epoch, 1);
  if (rc) return rc;
  if (!(D_z > 0.0)) return fail(ctx, CHOMP_ERR_ARG, "cell: D_z");
  const ProjLayout& L = ctx->proj.L;
  const CellPlan P = cell_plan(ctx->cfg.divmax, ctx->L.NK, L, n, ctx->tune[CHOMP_TUNE_CELL_ONE_KERNEL],
                               false);
  if (!P.deep_fits) return fail(ctx, CHOMP_ERR_ARG, "cell: halo_npoints too large for k_cell_deep");
  HIPCHK(hipSetDevice(ctx->device));
  rc = prepare_extrapolation(ctx, which, epoch, 1);
  if (rc) return rc;
  const double* din;
  double* dout;
  st.in(ell, n, &din);
  st.out(out, n, &dout);
  rc = st.place();
  if (rc) return rc;
  // the chi-only factors of the integrand on the Romberg nodes first (CellPlan: the node table,
  // then one slab -- the spectrum table and the hand-over of k_cell to k_cell_deep)
  const int LT = P.LT, split = P.split;
  const size_t sh = P.sh;
  rc = ensure(ctx, ctx->d_cnodes, P.doubles(1));
  if (rc) return rc;
  double* state = ctx->d_cnodes + P.state_at;
  int* deep = reinterpret_cast<int*>(ctx->d_cnodes + P.deep_at);
  hipLaunchKernelGGL(k_cell_nodes, dim3(P.gnodes), dim3(256), P.sh_nodes, ctx->stream, L,
                     ctx->proj.d_pd, ctx->proj.d_tab, D_z, LT, ctx->d_cnodes, deep, 1, (size_t)0);
  // ... and the spectrum itself on a uniform ln k grid (no-wiggle spectra); levels beyond
  // kCellSplitLevel by k_cell_deep (CHOMP_TUNE_CELL_ONE_KERNEL: all in k_cell)
  double* pk_tab = ctx->with_bao ? nullptr : ctx->d_cnodes + P.pk_at;
  rc = with_flag(which & CHOMP_P_HALOFIT, ctx->with_bao, [&](auto HF, auto BAO) {
    if (pk_tab)
      hipLaunchKernelGGL((k_cell_ptab<HF, BAO>), dim3((kPTabN + 256) / 256), dim3(256),
                         (size_t)(12 * (ctx->L.NK - 1)) * sizeof(double), ctx->stream, ctx->cfg,
                         ctx->L, ctx->d_epochs, (int)epoch, ctx->d_tab, which, pk_tab);
    if (P.four) {   // (four multipoles to a block)
      hipLaunchKernelGGL((k_cell4<HF, BAO>), dim3((unsigned)((n + 3) / 4)), dim3(256), sh,
                         ctx->stream, ctx->cfg, ctx->L, L, ctx->d_epochs, (int)epoch,
                         ctx->d_tab, which, ctx->proj.d_pd, ctx->proj.d_tab, D_z, din, (int)n,
                         dout, ctx->d_cnodes, LT, pk_tab, split, deep, state);
    } else {   // (no level beyond the node table in k_cell: the lean instance)
      with_flag(split > LT, [&](auto BEYOND) {
        hipLaunchKernelGGL((k_cell<HF, BAO, BEYOND>), dim3((unsigned)n), dim3(256), sh, ctx->stream,
                           ctx->cfg, ctx->L, L, ctx->d_epochs, (int)epoch, ctx->d_tab, which,
                           ctx->proj.d_pd, ctx->proj.d_tab, D_z, din, dout, ctx->d_cnodes, LT,
                           pk_tab, split, deep, state);
      });
    }
    if (split >= ctx->cfg.divmax) return CHOMP_OK;
    const int rcl = lds_opt_in(ctx, &k_cell_deep<HF, BAO>, P.deep_lds);
    if (rcl) return rcl;
    hipLaunchKernelGGL((k_cell_deep<HF, BAO>), dim3(P.gdeep), dim3(kCellDeepThreads), P.shd,
                       ctx->stream, ctx->cfg, ctx->L, L, ctx->d_epochs, (int)epoch,
                       ctx->d_tab, which, ctx->proj.d_pd, ctx->proj.d_tab, D_z, din, dout,
                       ctx->d_cnodes, LT, pk_tab, split, deep, state);
    return CHOMP_OK;
  });
  if (rc) return rc;
  return st.finish();
}

int chomp_wtheta(chomp_ctx* ctx, int which, size_t epoch, double k_min, double k_max, double D_z,
                 const double* theta, size_t n, double* out, int mem) {
  StageRange range_(ctx, "chomp:wtheta");
  if (!ctx) return CHOMP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  return wtheta_impl(ctx, which, epoch, k_min, k_max, D_z, theta, n, out, mem);
}

// The rows of a batched projection.  sets == nullptr (chomp_*_epochs): every epoch against the
// context's projection set-up with the one growth factor D_z.  Otherwise (chomp_*_sets): epoch
// epoch0 + e against set e of the last set-up of sets with growth D_zs[e], a host array.
struct ProjRows {
  const char *who, *single;
  const ProjSets* sets;
  double D_z;
  const double* D_zs;
};

// The set-up the rows need, then the scope, then (sets) a row per set.
static int rows_check(chomp_ctx* ctx, const ProjRows& R, int which, size_t n_epoch,
                      const char* fp64_note = nullptr) {
  if (R.sets ? R.sets->n == 0 : !ctx->proj.ready)
    return fail(ctx, CHOMP_ERR_STATE, std::string(R.who) + (R.sets ? " before kernel_setup_sets / kernel_setup_pairs"
                                                                    : " before kernel_setup"));
  const int rc = batch_scope(ctx, R.who, R.single, which, fp64_note);
  if (rc) return rc;
  if (R.sets && n_epoch != R.sets->n)
    return fail(ctx, CHOMP_ERR_ARG, std::string(R.who) + ": n_epoch is not the number of sets of the last "
                                                         "kernel_setup_sets / kernel_setup_pairs");
  return CHOMP_OK;
}

static bool rows_growth_ok(const ProjRows& R, size_t n_epoch) {
  if (!R.sets) return R.D_z > 0.0;
  for (size_t e = 0; e < n_epoch; ++e)
    if (!(R.D_zs[e] > 0.0)) return false;
  return true;
}

// st.place() with (sets) the per-row growth factors behind it on the device: D_zs is a host array
// whatever `mem` says, so it goes through the scratch segment.  *dD: null without sets.
static int rows_place(chomp_ctx* ctx, Staging& st, const ProjRows& R, size_t n_epoch, const double** dD) {
  *dD = nullptr;
  const int rc = st.place(R.sets ? n_epoch : 0);
  if (rc || !R.sets) return rc;
  *dD = st.scratch;
  HIPCHK(hipMemcpyAsync(st.scratch, R.D_zs, n_epoch * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  return CHOMP_OK;
}

// The chunked driver of chomp_wtheta_epochs and chomp_wtheta_sets: the three launches of
// wtheta_impl with an epoch axis -- the _epochs kernels, or the _sets kernels with the chunk's
// first set and growth factor -- the epochs worked off in chunks that reuse one work buffer
// (layout: chomp_proj_kernels.h, "The epoch axis"; the sizes and the route: WthPlan).
static int wtheta_rows(chomp_ctx* ctx, const ProjRows& R, int which, size_t epoch0, size_t n_epoch,
                       double k_min, double k_max, const double* theta, size_t n, double* out, int mem) {
  int rc = batch_args(ctx, R.who, theta && out && (!R.sets || R.D_zs), n, n_epoch);
  if (rc) return rc;
  Staging st(ctx, mem, R.who);
  if (st.rc) return st.rc;
  rc = rows_check(ctx, R, which, n_epoch);
  if (rc) return rc;
  rc = check_power(ctx, which, epoch0, n_epoch);
  if (rc) return rc;
  const bool range_ok = k_min > 0.0 && k_max > k_min;
  if (!R.sets) {
    if (!range_ok || !rows_growth_ok(R, n_epoch)) return fail(ctx, CHOMP_ERR_ARG, std::string(R.who) + ": k range / D_z");
  } else {
    if (!range_ok) return fail(ctx, CHOMP_ERR_ARG, std::string(R.who) + ": k range");
    if (!rows_growth_ok(R, n_epoch)) return fail(ctx, CHOMP_ERR_ARG, std::string(R.who) + ": D_z");
  }
  HIPCHK(hipSetDevice(ctx->device));
  if (!R.sets) { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  const double *din, *dD;
  double* dout;
  st.in(theta, n, &din);
  st.out(out, n * n_epoch, &dout);
  rc = rows_place(ctx, st, R, n_epoch, &dD);
  if (rc) return rc;
  const ProjLayout& L = R.sets ? R.sets->L : ctx->proj.L;
  const ProjDev& host = R.sets ? R.sets->host : ctx->proj.host;
  const WthPlan P = wth_plan(ctx->cfg.divmax, ctx->L.NK, L, host.ln_kt_min, host.ln_kt_max, k_min,
                             k_max, ctx->tune[CHOMP_TUNE_WTHETA_DIRECT]);
  const int LT = P.LT, nseg = P.nseg;
  const size_t stride = P.stride, pstride = (size_t)L.total;
  const size_t chunk = epoch_chunk(ctx, n_epoch);
  rc = ensure(ctx, ctx->d_wnodes, stride * chunk);
  if (rc) return rc;
  double* rec = ctx->d_wnodes + P.rec_at;                   // (of the chunk's first epoch)
  double* segtot = ctx->d_wnodes + P.tot_at;
  constexpr bool HF = false, BAO = false;
  for (size_t c0 = 0; c0 < n_epoch; c0 += chunk) {          // (the scratch is reused in stream order)
    const unsigned E = (unsigned)std::min(chunk, n_epoch - c0);
    const int e0 = (int)(epoch0 + c0);
    double* o = dout + c0 * n;
    const ProjDev* pd = R.sets ? R.sets->d_pd + c0 : ctx->proj.d_pd;   // (sets: the chunk's first set)
    const double* ptab = R.sets ? R.sets->d_tab + c0 * pstride : ctx->proj.d_tab;
    if (R.sets)
      hipLaunchKernelGGL((k_wtheta_nodes_sets<HF, BAO>), dim3(P.gnodes, E), dim3(256), P.sh_nodes,
                         ctx->stream, ctx->cfg, ctx->L, ctx->d_epochs, e0, ctx->d_tab, which, k_min,
                         k_max, dD + c0, LT, ctx->d_wnodes, stride);
    else
      hipLaunchKernelGGL((k_wtheta_nodes_epochs<HF, BAO>), dim3(P.gnodes, E), dim3(256), P.sh_nodes,
                         ctx->stream, ctx->cfg, ctx->L, ctx->d_epochs, e0, ctx->d_tab, which, k_min,
                         k_max, R.D_z, LT, ctx->d_wnodes, stride);
    if (P.fast) {
      hipLaunchKernelGGL(k_wtheta_moments_epochs, dim3((unsigned)nseg, (unsigned)LT, kWthParts * E),
                         dim3(256), 0, ctx->stream, ctx->d_wnodes, LT, nseg, std::log(k_min),
                         std::log(k_max), rec, segtot, stride);
      if (R.sets)
        hipLaunchKernelGGL(k_wtheta_fast_sets, dim3((unsigned)n, E), dim3(256), 0, ctx->stream,
                           ctx->cfg, L, pd, ptab, pstride, k_min, k_max, din, o, ctx->d_wnodes, rec,
                           segtot, LT, nseg, stride);
      else
        hipLaunchKernelGGL(k_wtheta_fast_epochs, dim3((unsigned)n, E), dim3(256), 0, ctx->stream,
                           ctx->cfg, L, pd, ptab, k_min, k_max, din, o, ctx->d_wnodes, rec, segtot,
                           LT, nseg, stride);
    } else if (R.sets) {
      hipLaunchKernelGGL((k_wtheta_sets<HF, BAO>), dim3((unsigned)n, E), dim3(64 * kWthetaNW), P.sh,
                         ctx->stream, ctx->cfg, ctx->L, L, ctx->d_epochs, e0, ctx->d_tab, which, pd,
                         ptab, pstride, k_min, k_max, dD + c0, din, o, ctx->d_wnodes, LT, stride);
    } else {
      hipLaunchKernelGGL((k_wtheta_epochs<HF, BAO>), dim3((unsigned)n, E), dim3(64 * kWthetaNW), P.sh,
                         ctx->stream, ctx->cfg, ctx->L, L, ctx->d_epochs, e0, ctx->d_tab, which, pd,
                         ptab, k_min, k_max, R.D_z, din, o, ctx->d_wnodes, LT, stride);
    }
  }
  return st.finish();
}

// w(theta) of n_epoch epochs that share the projection set-up, the k range and D_z (an HOD design
// or chain at one cosmology).
int chomp_wtheta_epochs(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, double k_min,
                        double k_max, double D_z, const double* theta, size_t n, double* out,
                        int mem) {
  StageRange range_(ctx, "chomp:wtheta_epochs");
  if (!ctx) return CHOMP_ERR_ARG;
  const ProjRows R = {"wtheta_epochs", "chomp_wtheta", nullptr, D_z, nullptr};
  return wtheta_rows(ctx, R, which, epoch0, n_epoch, k_min, k_max, theta, n, out, mem);
}

// w(theta) of n_epoch epochs, epoch epoch0 + e against projection set e of the last set-up of
// sets with growth D_z[e] (a cosmology design or chain: the loop of
// set_cosmology + correlation, correlation.py:161-171 per point): chomp_wtheta_epochs with a
// per-row set and growth factor -- its scope, routes, chunks and work buffer.
int chomp_wtheta_sets(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, double k_min,
                      double k_max, const double* D_z, const double* theta, size_t n, double* out,
                      int mem) {
  StageRange range_(ctx, "chomp:wtheta_sets");
  if (!ctx) return CHOMP_ERR_ARG;
  const ProjRows R = {"wtheta_sets", "chomp_wtheta", &ctx->sets, 0.0, D_z};
  return wtheta_rows(ctx, R, which, epoch0, n_epoch, k_min, k_max, theta, n, out, mem);
}

int chomp_cell(chomp_ctx* ctx, int which, size_t epoch, double D_z, const double* ell, size_t n,
               double* out, int mem) {
  StageRange range_(ctx, "chomp:cell");
  if (!ctx) return CHOMP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  return cell_impl(ctx, which, epoch, D_z, ell, n, out, mem);
}

// The chunked driver of chomp_cell_epochs and chomp_cell_sets: the launches of cell_impl with an
// epoch axis, the epochs worked off in chunks that reuse the slabs of one work buffer (the sizes,
// the split and the route: CellPlan).  Without sets ONE chi-only node table serves the call
// (chomp_proj_kernels.h, "The epoch axis" of C_l); with sets every row has its own, built with the
// chunk ("The set axis of C_l").
static int cell_rows(chomp_ctx* ctx, const ProjRows& R, int which, size_t epoch0, size_t n_epoch,
                     const double* ell, size_t n, double* out, int mem) {
  int rc = batch_args(ctx, R.who, ell && out && (!R.sets || R.D_zs), n, n_epoch);
  if (rc) return rc;
  Staging st(ctx, mem, R.who);
  if (st.rc) return st.rc;
  rc = rows_check(ctx, R, which, n_epoch, "no narrowed precision mode evaluates C_l");
  if (rc) return rc;
  rc = check_power(ctx, which, epoch0, n_epoch);
  if (rc) return rc;
  if (!rows_growth_ok(R, n_epoch)) return fail(ctx, CHOMP_ERR_ARG, std::string(R.who) + ": D_z");
  const ProjLayout& L = R.sets ? R.sets->L : ctx->proj.L;
  const CellPlan P = cell_plan(ctx->cfg.divmax, ctx->L.NK, L, n, ctx->tune[CHOMP_TUNE_CELL_ONE_KERNEL],
                               R.sets != nullptr);
  if (!P.deep_fits) return fail(ctx, CHOMP_ERR_ARG, std::string(R.who) + ": halo_npoints too large for k_cell_deep");
  HIPCHK(hipSetDevice(ctx->device));
  if (!R.sets) { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  const double *din, *dD;
  double* dout;
  st.in(ell, n, &din);
  st.out(out, n * n_epoch, &dout);
  rc = rows_place(ctx, st, R, n_epoch, &dD);
  if (rc) return rc;
  const int LT = P.LT, split = P.split;
  const size_t stride = P.stride, pstride = (size_t)L.total;
  const size_t chunk = epoch_chunk(ctx, n_epoch);
  rc = ensure(ctx, ctx->d_cnodes, P.doubles(chunk));
  if (rc) return rc;
  double* pk_tab = ctx->d_cnodes + P.pk_at;                 // (of the chunk's first row)
  double* state = ctx->d_cnodes + P.state_at;
  int* deep = reinterpret_cast<int*>(ctx->d_cnodes + P.deep_at);
  constexpr bool HF = false, BAO = false;
  if (!R.sets)                      // (also empties the deep lists of the first chunk)
    hipLaunchKernelGGL(k_cell_nodes, dim3(P.gnodes), dim3(256), P.sh_nodes, ctx->stream, L,
                       ctx->proj.d_pd, ctx->proj.d_tab, R.D_z, LT, ctx->d_cnodes, deep, (int)chunk,
                       2 * stride);
  if (split < ctx->cfg.divmax) {
    rc = R.sets ? lds_opt_in(ctx, &k_cell_deep_sets<HF, BAO>, P.deep_lds)
                : lds_opt_in(ctx, &k_cell_deep_epochs<HF, BAO>, P.deep_lds);
    if (rc) return rc;
  }
  for (size_t c0 = 0; c0 < n_epoch; c0 += chunk) {          // (the slabs are reused in stream order)
    const unsigned E = (unsigned)std::min(chunk, n_epoch - c0);
    const int e0 = (int)(epoch0 + c0);
    double* o = dout + c0 * n;
    const ProjDev* pd = R.sets ? R.sets->d_pd + c0 : ctx->proj.d_pd;   // (sets: the chunk's first set)
    const double* ptab = R.sets ? R.sets->d_tab + c0 * pstride : ctx->proj.d_tab;
    if (R.sets)                     // (... and empties the rows' deep lists)
      hipLaunchKernelGGL(k_cell_nodes_sets, dim3(P.gnodes, E), dim3(256), P.sh_nodes, ctx->stream, L,
                         pd, ptab, pstride, dD + c0, LT, ctx->d_cnodes, deep, stride);
    hipLaunchKernelGGL((k_cell_ptab_epochs<HF, BAO>), dim3((kPTabN + 256) / 256, E), dim3(256),
                       (size_t)(12 * (ctx->L.NK - 1)) * sizeof(double), ctx->stream, ctx->cfg,
                       ctx->L, ctx->d_epochs, e0, ctx->d_tab, which, pk_tab,
                       !R.sets && c0 ? deep : (int*)nullptr, stride);
    if (P.four) {                   // (four multipoles to a block)
      if (R.sets)
        hipLaunchKernelGGL((k_cell4_sets<HF, BAO>), dim3((unsigned)((n + 3) / 4), E), dim3(256), P.sh,
                           ctx->stream, ctx->cfg, ctx->L, L, ctx->d_epochs, e0, ctx->d_tab, which,
                           pd, ptab, pstride, dD + c0, din, (int)n, o, ctx->d_cnodes, LT, pk_tab,
                           split, deep, state, stride);
      else
        hipLaunchKernelGGL((k_cell4_epochs<HF, BAO>), dim3((unsigned)((n + 3) / 4), E), dim3(256), P.sh,
                           ctx->stream, ctx->cfg, ctx->L, L, ctx->d_epochs, e0, ctx->d_tab, which,
                           pd, ptab, R.D_z, din, (int)n, o, ctx->d_cnodes, LT, pk_tab, split, deep,
                           state, stride);
    } else {
      with_flag(split > LT, [&](auto BEYOND) {
        if (R.sets)
          hipLaunchKernelGGL((k_cell_sets<HF, BAO, BEYOND>), dim3((unsigned)n, E), dim3(256), P.sh,
                             ctx->stream, ctx->cfg, ctx->L, L, ctx->d_epochs, e0, ctx->d_tab, which,
                             pd, ptab, pstride, dD + c0, din, o, ctx->d_cnodes, LT, pk_tab, split,
                             deep, state, stride);
        else
          hipLaunchKernelGGL((k_cell_epochs<HF, BAO, BEYOND>), dim3((unsigned)n, E), dim3(256), P.sh,
                             ctx->stream, ctx->cfg, ctx->L, L, ctx->d_epochs, e0, ctx->d_tab, which,
                             pd, ptab, R.D_z, din, o, ctx->d_cnodes, LT, pk_tab, split, deep, state,
                             stride);
      });
    }
    if (split >= ctx->cfg.divmax) continue;
    if (R.sets)
      hipLaunchKernelGGL((k_cell_deep_sets<HF, BAO>), dim3(P.gdeep, E), dim3(kCellDeepThreads), P.shd,
                         ctx->stream, ctx->cfg, ctx->L, L, ctx->d_epochs, e0, ctx->d_tab, which,
                         pd, ptab, pstride, dD + c0, din, (int)n, o, ctx->d_cnodes, LT, pk_tab,
                         split, deep, state, stride);
    else
      hipLaunchKernelGGL((k_cell_deep_epochs<HF, BAO>), dim3(P.gdeep, E), dim3(kCellDeepThreads), P.shd,
                         ctx->stream, ctx->cfg, ctx->L, L, ctx->d_epochs, e0, ctx->d_tab, which,
                         pd, ptab, R.D_z, din, (int)n, o, ctx->d_cnodes, LT, pk_tab, split, deep,
                         state, stride);
  }
  return st.finish();
}

// C_l of n_epoch epochs that share the projection set-up and D_z (an HOD design or chain at one
// cosmology).
int chomp_cell_epochs(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, double D_z,
                      const double* ell, size_t n, double* out, int mem) {
  StageRange range_(ctx, "chomp:cell_epochs");
  if (!ctx) return CHOMP_ERR_ARG;
  const ProjRows R = {"cell_epochs", "chomp_cell", nullptr, D_z, nullptr};
  return cell_rows(ctx, R, which, epoch0, n_epoch, ell, n, out, mem);
}

// C_l of n_epoch epochs, epoch epoch0 + e against projection set e of the last set-up of sets with
// growth D_z[e] (the kernels of a tomographic analysis, or a cosmology design or chain over C_l):
// chomp_cell_epochs with a per-row set, growth factor and chi-only node table -- its scope, routes
// and chunks.
int chomp_cell_sets(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, const double* D_z,
                    const double* ell, size_t n, double* out, int mem) {
  StageRange range_(ctx, "chomp:cell_sets");
  if (!ctx) return CHOMP_ERR_ARG;
  const ProjRows R = {"cell_sets", "chomp_cell", &ctx->sets, 0.0, D_z};
  return cell_rows(ctx, R, which, epoch0, n_epoch, ell, n, out, mem);
}

// w(theta) and C_l of one set-up in one call (configs[3], [4]: both observables of a survey).
// Neither needs anything the other produces -- different node tables, different scratch -- so
// with device buffers C_l runs on the side stream beside w(theta) and is joined before the
// call returns: in the order of the context's stream the call behaves like the two calls in
// sequence, and returns identical numbers.  Host buffers share the staging area and
// extrapolated spectra their constants' refresh: those run one after the other.
int chomp_wtheta_cell(chomp_ctx* ctx, int which, size_t epoch, double k_min, double k_max,
                      double D_z, const double* theta, size_t n_theta, double* w_out,
                      const double* ell, size_t n_ell, double* c_out, int mem) {
  StageRange range_(ctx, "chomp:wtheta_cell");
  if (!ctx) return CHOMP_ERR_ARG;
  { const int rcm = check_mem(ctx, mem, "wtheta_cell"); if (rcm) return rcm; }
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  int rc = CHOMP_OK;
  bool forked = false;
  if (mem == CHOMP_DEVICE && !(which & CHOMP_P_EXTRAPOLATE)) {
    SideScope side(ctx, &ctx->ev_side_done);
    rc = side.begin();
    if (rc) return rc;
    if (side.on()) {
      forked = true;
      rc = cell_impl(ctx, which, epoch, D_z, ell, n_ell, c_out, mem);
      side.end();
    }
  }
  if (!forked) rc = cell_impl(ctx, which, epoch, D_z, ell, n_ell, c_out, mem);
  const int rcw = rc ? rc : wtheta_impl(ctx, which, epoch, k_min, k_max, D_z, theta, n_theta, w_out, mem);
  if (forked) HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_side_done, 0));   // (joined in any case)
  return rcw;
}

// ---------------------------------------------------------------------------
// What the covariance calls share (DESIGN.md, "One set of checks, plans and tails behind the
// covariance calls").  Every message is composed from the call's name on the failure path only.
// (templates have C++ linkage: extern "C++" inside this file's extern "C")
// ---------------------------------------------------------------------------
// The dynamic LDS of a launch beside the kernel's static LDS fits the 64 kB a workgroup may use.
extern "C++" template <class Kernel>
static bool fits_lds(Kernel* kernel, size_t dynamic_bytes) {
  hipFuncAttributes attr;
  if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kernel)) != hipSuccess) return false;
  return dynamic_bytes + attr.sharedSizeBytes <= 64 * 1024;
}
// ... of the instance of a kernel template that `flag` selects.
extern "C++" template <class Kernel>
static bool fits_lds(bool flag, Kernel* on, Kernel* off, size_t dynamic_bytes) {
  return flag ? fits_lds(on, dynamic_bytes) : fits_lds(off, dynamic_bytes);
}

// One kind of table (or run of scalars) of a slab on its way back to the host: `count` tables
// of n doubles, the t-th from base + at[t] to out + t * n (out == nullptr: not asked for).
struct SlabRows {
  double* out;
  const int* at;
  int count;
  size_t n;
};
// Synchronise (unless the caller has), then copy the rows back in the order given; nothing at
// all when nothing is asked for.
static int slab_read(chomp_ctx* ctx, const double* base, std::initializer_list<SlabRows> rows,
                     bool synced = false) {
  bool any = false;
  for (const SlabRows& r : rows) any = any || r.out;
  if (!any) return CHOMP_OK;
  if (!synced) HIPCHK(hipStreamSynchronize(ctx->stream));
  for (const SlabRows& r : rows)
    for (int t = 0; r.out && t < r.count; ++t)
      HIPCHK(hipMemcpy(r.out + (size_t)t * r.n, base + r.at[t], r.n * sizeof(double), hipMemcpyDeviceToHost));
  return CHOMP_OK;
}

// The windows behind a kernel_ssc / kernel_NG / CovarianceFourier state: the context's own
// kernel_setup, or (four) the two slots of its cross block.
static CovSrc cov_src(const chomp_ctx* ctx, bool four) {
  const ProjState& P = ctx->proj;
  if (!four) return CovSrc{P.d_pd, P.d_tab, nullptr, nullptr};
  const CrossState& X = ctx->cross;
  return CovSrc{reinterpret_cast<const ProjDev*>(X.d + X.C.pd[0]), X.d + X.C.ptab[0],
                reinterpret_cast<const ProjDev*>(X.d + X.C.pd[1]), X.d + X.C.ptab[1]};
}

// A cross block's slots are staged and of the configuration of L; with `overlap`, their four
// windows have a redshift in common as well.
static int check_cross_slots(chomp_ctx* ctx, const ProjLayout& L, const char* what, bool overlap) {
  const CrossState& X = ctx->cross;
  if (!X.staged[0] || !X.staged[1])
    return fail(ctx, CHOMP_ERR_STATE, std::string(what) + " before covariance_cross_stage of both slots");
  if (X.C.pd[0] - X.C.htab[0] != ctx->L.stride || X.C.N != L.NKT ||
      X.C.ptab[1] - X.C.ptab[0] < L.total)
    return fail(ctx, CHOMP_ERR_STATE, std::string(what) + ": the snapshots are of another configuration");
  if (overlap && !(std::max(X.z_min[0], X.z_min[1]) < std::min(X.z_max[0], X.z_max[1])))
    return fail(ctx, CHOMP_ERR_SCOPE, std::string(what) + ": the four windows have no redshift in common "
                                                          "(kernel.py:910-916 would give z_min >= z_max)");
  return CHOMP_OK;
}

// *sh: the dynamic LDS of the knots of a cross block (k_cov_cross_knots, k_cov_blocks_knots), in
// bytes; refused beyond 64 kB.
static int cross_lds_bytes(chomp_ctx* ctx, const ProjLayout& L, const char* who, size_t* sh) {
  *sh = (size_t)cov_cross_lds_doubles(ctx->L.NK, L) * sizeof(double);
  if (*sh > 64 * 1024)
    return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": halo/cosmo/window_npoints too large for "
                                                       "the two spectra and four windows of a cross block");
  return CHOMP_OK;
}

// The dynamic LDS of the Gaussian term's launches: ln K and the splines of `tables` tables.
static size_t gaussian_lds_bytes(int N, int tables) {
  return (size_t)(N + 4 * tables * (N - 1)) * sizeof(double);
}
// What the three Gaussian calls ask of (j0_limit, area) and of host angles theta[2 n]; each call
// keeps what it does between the two.
static int gaussian_scalars(chomp_ctx* ctx, const char* who, double j0_limit, double area) {
  if (!(j0_limit > 0.0) || !(area > 0.0))
    return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": j0_limit and area must be positive");
  return CHOMP_OK;
}
static int gaussian_theta(chomp_ctx* ctx, const char* who, bool host, const double* theta, size_t n) {
  for (size_t i = 0; host && i < 2 * n; ++i)
    if (!(theta[i] > 0.0)) return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": theta must be positive");
  return CHOMP_OK;
}

// What the block-axis calls ask of the sets: a set-up of n_corr sets of order 0 and at most 65535
// blocks; with `overlap` (the super-sample calls), in every block windows with a redshift in
// common as well (check_cross_slots' rule, from the host's ranges: nothing is launched).
static int blocks_check(chomp_ctx* ctx, const char* who, size_t n_corr, bool overlap) {
  const ProjSets& S = ctx->sets;
  const auto refuse = [&](int code, const std::string& text) { return fail(ctx, code, std::string(who) + text); };
  if (S.n == 0) return refuse(CHOMP_ERR_STATE, " before kernel_setup_pairs / kernel_setup_sets");
  if (S.n != n_corr)
    return refuse(CHOMP_ERR_STATE, ": n_corr is not the number of sets of the last "
                                   "kernel_setup_pairs / kernel_setup_sets");
  if (S.host.order != 0)
    return refuse(CHOMP_ERR_STATE, ": the sets are of Bessel order 2 (the covariance of "
                                   "w(theta) takes the windows of a Kernel, order 0)");
  if (n_corr * (n_corr + 1) / 2 > 65535)                  // (n_corr <= kProjSetsMax)
    return refuse(CHOMP_ERR_ARG, ": more than 65535 blocks (a grid's z dimension)");
  for (size_t i = 0; overlap && i < n_corr; ++i)
    for (size_t j = i; j < n_corr; ++j)
      if (!(std::max(ctx->sets_z_min[i], ctx->sets_z_min[j]) <
            std::min(ctx->sets_z_max[i], ctx->sets_z_max[j])))
        return refuse(CHOMP_ERR_SCOPE, ": block (" + std::to_string(i) + ", " + std::to_string(j) +
                                       "): the four windows have no redshift in common "
                                       "(kernel.py:910-916 would give z_min >= z_max)");
  return CHOMP_OK;
}

// The index block of n_corr correlations (chomp_proj_kernels.h, chomp_cov_kernels.h): epoch |
// (i, j) and, with `lists`, | the diagonal blocks | the cross blocks.  epoch == nullptr: epoch c
// for correlation c (the range call reads no epoch; with these the block is most often the one
// the call behind it sends).
static std::vector<int> blocks_index(size_t n_corr, const size_t* epoch, bool lists) {
  const size_t n_blocks = n_corr * (n_corr + 1) / 2;
  std::vector<int> index(n_corr + (lists ? 3 : 2) * n_blocks);
  for (size_t c = 0; c < n_corr; ++c) index[c] = epoch ? (int)epoch[c] : (int)c;
  int* diag = lists ? index.data() + n_corr + 2 * n_blocks : nullptr;
  int* cross = lists ? diag + n_corr : nullptr;
  size_t b = 0;
  for (size_t i = 0; i < n_corr; ++i)
    for (size_t j = i; j < n_corr; ++j, ++b) {
      index[n_corr + 2 * b] = (int)i;
      index[n_corr + 2 * b + 1] = (int)j;
      if (lists) *(i == j ? diag : cross)++ = (int)b;
    }
  return index;
}
// ... in a state's device buffer (grown if need be), through its staging block.
static int blocks_index_upload(chomp_ctx* ctx, StagedBuffer<int>& d_index, const std::vector<int>& index) {
  const int rc = ensure(ctx, d_index, index.size());
  if (rc) return rc;
  return upload(ctx, d_index, index.data(), index.size() * sizeof(int));
}

// One call on the block axis (chomp_covariance_blocks, _ssc_blocks, _ng_blocks): its staged
// arrays, the sizes n_corr gives and where the sets of the last set-up lie.  The steps are made
// in the order written here; a call makes its own refusals and launches between them.
// (member templates need C++ linkage too)
extern "C++" struct BlocksCall {
  chomp_ctx* ctx;
  const char* who;
  Staging st;
  const ProjSets& S;
  const ProjLayout& L;                   // the sets'
  const size_t n_corr, n_pairs, n_blocks, n_cross, pstride;
  const int nc;
  const unsigned Z;                      // n_blocks, as a grid's extent
  const int *d_index = nullptr, *d_diag = nullptr, *d_cross = nullptr;   // (begin)
  double *d_knots = nullptr, *d_lev = nullptr;
  const double* d_theta = nullptr;       // (place)
  double* d_out = nullptr;

  BlocksCall(chomp_ctx* c, const char* w, int mem, size_t n, size_t pairs)
      : ctx(c), who(w), st(c, mem, w), S(c->sets), L(S.L), n_corr(n), n_pairs(pairs),
        n_blocks(n * (n + 1) / 2), n_cross(n_blocks - n), pstride((size_t)L.total), nc((int)n),
        Z((unsigned)n_blocks) {}
  int refuse(int code, const std::string& text) const { return fail(ctx, code, std::string(who) + text); }
  // What every call refuses first (the null context aside): "bad args" (`args`: its arrays are
  // there), a `mem` that Staging does not know, blocks_check.
  int head(bool args, bool overlap) {
    if (!args || n_corr == 0 || n_pairs == 0) return refuse(CHOMP_ERR_ARG, ": bad args");
    if (st.rc) return st.rc;
    return blocks_check(ctx, who, n_corr, overlap);
  }
  // check(c): the term's refusal of correlation c's epoch, its text in ctx->err.
  template <class Check>
  int epochs(Check&& check) {
    for (size_t c = 0; c < n_corr; ++c) {
      const int rc = check(c);
      if (rc) return refuse(rc, ": correlation " + std::to_string(c) + ": " + ctx->err);
    }
    return CHOMP_OK;
  }
  // Behind the last refusal: the state's last result is given up, its buffers grown to `slabs`
  // doubles of slabs and `kb` of k_b knots and levels, the index block (with the lists) sent.
  int begin(TermBlocksState& B, size_t slabs, size_t kb, const size_t* epoch) {
    B.n_corr = 0;
    int rc = ensure(ctx, B.d, slabs);
    if (!rc) rc = ensure(ctx, B.d_kb, kb);
    if (!rc) rc = blocks_index_upload(ctx, B.d_index, blocks_index(n_corr, epoch, true));
    if (rc) return rc;
    d_index = B.d_index;
    d_diag = d_index + n_corr + 2 * n_blocks;
    d_cross = d_diag + n_corr;
    d_knots = B.d_kb;
    d_lev = d_knots + kb / 2;
    return CHOMP_OK;
  }
  // theta[2 n_pairs] in, out[n_blocks][n_pairs] out.
  int place(const double* theta, double* out) {
    st.in(theta, 2 * n_pairs, &d_theta);
    st.out(out, n_blocks * n_pairs, &d_out);
    return st.place();
  }
  // The two instances of a term's prep or table kernel over slabs of layout T: <false> over the
  // list of diagonal blocks, then <true> over that of the cross blocks, if there are any.  Grid
  // (x, listed blocks), or (listed blocks) for x == 0; sh: the dynamic LDS of each; `more`: the
  // arguments behind the list.
  template <class Diag, class Cross, class Layout, class... More>
  void lists(Diag* diag, Cross* cross, unsigned x, const size_t (&sh)[2], const Layout& T,
             const More&... more) const {
    const auto grid = [x](size_t n) { return x ? dim3(x, (unsigned)n) : dim3((unsigned)n); };
    hipLaunchKernelGGL(diag, grid(n_corr), dim3(256), sh[0], ctx->stream, ctx->cfg, L, T, nc, S.d_pd,
                       S.d_tab, pstride, d_index, d_diag, more...);
    if (n_cross)
      hipLaunchKernelGGL(cross, grid(n_cross), dim3(256), sh[1], ctx->stream, ctx->cfg, L, T, nc,
                         S.d_pd, S.d_tab, pstride, d_index, d_cross, more...);
  }
  // The tail: every block's pairs from their k_b knots, and the state readable again.
  int finish(TermBlocksState& B, size_t sh_outer, double area) {
    hipLaunchKernelGGL(k_ssc_blocks_outer, dim3((unsigned)n_pairs, Z), dim3(256), sh_outer,
                       ctx->stream, ctx->cfg, area, d_knots, d_out);
    HIPCHK(hipGetLastError());
    B.n_corr = n_corr;
    B.n_pairs = n_pairs;
    return st.finish();
  }
};

// One block of the last call of a term on the block axis, for chomp_covariance_<who>_table (host
// arrays, any may be NULL): info[7], the table and its levels [N, N] of layout T, scalar
// `extra_at` of the slab, and the block's k_b knots and levels.
extern "C++" template <class Layout>
static int term_blocks_table(chomp_ctx* ctx, const char* who, const TermBlocksState& B,
                             const Layout& T, size_t block, double* info, double* table,
                             double* levels, double* extra, int extra_at, double* kb_knots,
                             double* kb_levels) {
  if (B.n_corr == 0)
    return fail(ctx, CHOMP_ERR_STATE, std::string(who) + "_table before " + who);
  const size_t n_blocks = B.n_corr * (B.n_corr + 1) / 2;
  if (block >= n_blocks) return fail(ctx, CHOMP_ERR_ARG, std::string(who) + "_table: block");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int z_bar = T.scal + kSscZBar, z_min = T.scal + kSscZMin, at = T.scal + extra_at;
  const size_t NN = (size_t)T.N * T.N;
  const int rc = slab_read(ctx, B.d + block * (size_t)T.total,
                           {{info, &z_bar, 1, 3}, {info ? info + 3 : nullptr, &z_min, 1, 4},
                            {table, &T.tab, 1, NN}, {levels, &T.lev, 1, NN}, {extra, &at, 1, 1}}, true);
  if (rc) return rc;
  const size_t row = B.n_pairs * (size_t)ctx->cfg.kernel_npoints;
  if (kb_knots) HIPCHK(hipMemcpy(kb_knots, B.d_kb + block * row, row * sizeof(double), hipMemcpyDeviceToHost));
  if (kb_levels)
    HIPCHK(hipMemcpy(kb_levels, B.d_kb + (n_blocks + block) * row, row * sizeof(double), hipMemcpyDeviceToHost));
  return CHOMP_OK;
}

// The pairs of angles of chomp_covariance_ssc, _ssc_cross and _ng: what they refuse ...
static int pairs_check(chomp_ctx* ctx, const char* who, double area, size_t n) {
  if (!(area > 0.0)) return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": area must be positive");
  if (n > 65535) return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": at most 65535 pairs a call");
  return CHOMP_OK;
}
static int pairs_positive(chomp_ctx* ctx, const char* who, const double* theta, size_t n) {
  for (size_t i = 0; i < 2 * n; ++i)
    if (!(theta[i] > 0.0)) return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": arguments must be positive");
  return CHOMP_OK;
}
// ... their arrays on the device: theta[2 n], out[n], the k_b knots and their levels [n * NK]
// (k_ssc_outer reads the knots: staged even when not copied back) ...
struct PairArrays {
  const double* theta;
  double *out, *knots, *lev;
  void stage(Staging& st, const double* theta_, size_t n, int NK, double* out_, double* kb_knots,
             double* kb_levels) {
    st.in(theta_, 2 * n, &theta);
    st.out(out_, n, &out);
    st.out(kb_knots, n * NK, &knots);
    st.out(kb_levels, n * NK, &lev);
  }
};
// ... and the outer integral over the knots the call's own launches left, and the way back.
static int pairs_finish(chomp_ctx* ctx, Staging& st, const PairArrays& d, size_t n, size_t sh_outer,
                        double area) {
  hipLaunchKernelGGL(k_ssc_outer, dim3((unsigned)n), dim3(256), sh_outer, ctx->stream, ctx->cfg, area,
                     d.knots, d.out);
  return st.finish();
}

// The four evaluators of ln(k theta) pairs, chomp_kernel_{ssc,ng}_{raw,eval}: out[n] from
// ln_ktheta[2 n].  `ready`: the flag of ctx->proj the call needs, set by `setup`; max_n: the most
// points of a call (0: no bound); finite: the values are checked; launch(d_in, d_out) queues the
// kernel.
extern "C++" template <class Launch>
static int pair_eval(chomp_ctx* ctx, const char* who, const char* setup, bool ProjState::*ready,
                     size_t max_n, bool finite, const double* ln_ktheta, size_t n, double* out,
                     Launch launch) {
  if (!ctx || !ln_ktheta || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": bad args");
  if (!ctx->proj.ready || !(ctx->proj.*ready))
    return fail(ctx, CHOMP_ERR_STATE, std::string(who) + " before " + setup);
  if (max_n && n > max_n) return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": too many points");
  for (size_t i = 0; finite && i < 2 * n; ++i)
    if (!std::isfinite(ln_ktheta[i])) return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": ln(k theta) must be finite");
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  Staging st(ctx, CHOMP_HOST, who);
  const double* d_in;
  double* d_out;
  st.in(ln_ktheta, 2 * n, &d_in);
  st.out(out, n, &d_out);
  const int rc = st.place();
  if (rc) return rc;
  launch(d_in, d_out);
  return st.finish();
}

int chomp_covariance_table(chomp_ctx* ctx, int which, size_t epoch, double D_z, double* ln_K,
                           double* proj, double* levels, size_t n) {
  if (!ctx) return CHOMP_ERR_ARG;
  if (!ctx->proj.ready) return fail(ctx, CHOMP_ERR_STATE, "covariance_table before kernel_setup");
  int rc = check_power(ctx, which, epoch, 1);
  if (rc) return rc;
  if (!(D_z > 0.0)) return fail(ctx, CHOMP_ERR_ARG, "covariance_table: D_z");
  const ProjLayout& L = ctx->proj.L;
  const CovLayout C = make_cov_layout(L.NKT);
  if ((ln_K || proj || levels) && n != (size_t)C.N)
    return fail(ctx, CHOMP_ERR_ARG, "covariance_table: length must be kernel_npoints");
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  rc = prepare_extrapolation(ctx, which, epoch, 1);
  if (rc) return rc;
  ProjState& P = ctx->proj;
  P.cov_ready = false;
  HIPCHK((hipError_t)P.d_cov.once((size_t)C.total));
  const size_t sh = (size_t)(12 * (ctx->L.NK - 1) + ProjLds::doubles(L)) * sizeof(double);
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_cov_proj_knots<BAO>, dim3((unsigned)C.N), dim3(256), sh, ctx->stream,
                       ctx->cfg, ctx->L, L, C, ctx->d_epochs, (int)epoch, ctx->d_tab, which,
                       P.d_pd, P.d_tab, D_z, P.d_cov);
  });
  hipLaunchKernelGGL(k_cov_spline, dim3(1), dim3(64), 0, ctx->stream, C, P.d_cov);
  HIPCHK(hipGetLastError());
  P.cov_ready = true;
  const size_t N = (size_t)C.N;
  return slab_read(ctx, P.d_cov, {{ln_K, &C.ln_K, 1, N}, {proj, &C.proj, 1, N}, {levels, &C.lev, 1, N}});
}

int chomp_covariance_gaussian(chomp_ctx* ctx, double j0_limit, double area, double poisson_a,
                              double poisson_b, const double* theta, size_t n, double* out,
                              int mem) {
  if (!ctx || !theta || !out || n == 0)
    return fail(ctx, CHOMP_ERR_ARG, "covariance_gaussian: bad args");
  Staging st(ctx, mem, "covariance_gaussian");
  if (st.rc) return st.rc;
  if (!ctx->proj.cov_ready)
    return fail(ctx, CHOMP_ERR_STATE, "covariance_gaussian before covariance_table");
  int rc = gaussian_scalars(ctx, "covariance_gaussian", j0_limit, area);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  rc = gaussian_theta(ctx, "covariance_gaussian", st.host, theta, n);
  if (rc) return rc;
  const double* d_theta;
  double* d_out;
  st.in(theta, 2 * n, &d_theta);
  st.out(out, n, &d_out);
  rc = st.place();
  if (rc) return rc;
  const CovLayout C = make_cov_layout(ctx->proj.L.NKT);
  const size_t sh = gaussian_lds_bytes(C.N, 1);
  hipLaunchKernelGGL(k_cov_gaussian, dim3((unsigned)n), dim3(256), sh, ctx->stream, ctx->cfg, C,
                     ctx->proj.d_cov, ctx->d_j0, j0_limit, area, poisson_a, poisson_b, d_theta,
                     d_theta + n, d_out, (double*)nullptr);
  return st.finish();
}

// ---------------------------------------------------------------------------
// Gaussian cross-covariance of two w(theta): Covariance(corr_a, corr_b)
// ---------------------------------------------------------------------------
int chomp_covariance_cross_stage(chomp_ctx* ctx, int slot, chomp_ctx* src, int which,
                                 size_t epoch) {
  if (!ctx || !src) return fail(ctx, CHOMP_ERR_ARG, "covariance_cross_stage: bad args");
  if (slot < 0 || slot > 1) return fail(ctx, CHOMP_ERR_ARG, "covariance_cross_stage: slot must be 0 or 1");
  if (!src->proj.ready)
    return fail(ctx, CHOMP_ERR_STATE, "covariance_cross_stage: the source context has no kernel_setup");
  const bool windows_only = which == CHOMP_CROSS_WINDOWS;
  if (!windows_only) { const int rcp = check_power(src, which, epoch, 1); if (rcp) return fail(ctx, rcp, "covariance_cross_stage: source: " + src->err); }
  if (src->device != ctx->device)
    return fail(ctx, CHOMP_ERR_SCOPE, "covariance_cross_stage: both contexts must be on one device");
  if (std::memcmp(&src->cfg, &ctx->cfg, sizeof(chomp_config)) != 0 || src->with_bao != ctx->with_bao)
    return fail(ctx, CHOMP_ERR_SCOPE, "covariance_cross_stage: both contexts must share one "
                                      "configuration and transfer function");
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(src); if (rcj) return fail(ctx, rcj, "covariance_cross_stage: source: " + src->err); }
  if (!windows_only) { const int rce = prepare_extrapolation(src, which, epoch, 1); if (rce) return fail(ctx, rce, "covariance_cross_stage: source: " + src->err); }
  // (another context's stream is not ordered against this one: wait for what it holds before
  //  the copies, and for the copies before it may rewrite what they read)
  if (src != ctx) HIPCHK(hipStreamSynchronize(src->stream));
  CrossState& X = ctx->cross;
  const ProjLayout& L = src->proj.L;
  const CrossLayout C = make_cross_layout(L.NKT, src->L.stride, L.total);
  if (!X.d || X.C.total != C.total || X.C.htab[1] != C.htab[1] || X.C.ln_K != C.ln_K)
    X.staged[0] = X.staged[1] = false;                   // (another layout: both sides again)
  { bool moved = false;
    const int rce = ensure(ctx, X.d, (size_t)C.total, &moved); if (rce) return rce;
    if (moved) X.staged[0] = X.staged[1] = false; }
  X.C = C;
  X.ready = false;
  X.staged[slot] = false;
  // (the kernel_ssc / kernel_NG states of the block's four windows were built from the slots)
  if (ctx->proj.ssc_four) ctx->proj.ssc_prep = ctx->proj.ssc_ready = false;
  if (ctx->proj.ng_four) ctx->proj.ng_prep = ctx->proj.ng_ready = false;
  const auto copy = [&](int off, const void* from, size_t doubles) {
    return hipMemcpyAsync(X.d + off, from, doubles * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
  };
  if (!windows_only) {
    HIPCHK(copy(C.ep[slot], src->d_epochs + epoch, kEpochDoubles));
    HIPCHK(copy(C.htab[slot], src->d_tab + epoch * (size_t)src->L.stride, (size_t)src->L.stride));
  }
  HIPCHK(copy(C.pd[slot], src->proj.d_pd, kProjDoubles));
  HIPCHK(copy(C.ptab[slot], src->proj.d_tab, (size_t)L.total));
  if (src != ctx) HIPCHK(hipStreamSynchronize(ctx->stream));
  X.staged[slot] = true;
  X.which[slot] = which;
  {   // what chomp_covariance_ssc_cross asks of the snapshot: the families of the response
    const unsigned need = (1u << F_HM) | (1u << F_PPMM) | (1u << F_I12);
    X.response[slot] = !windows_only && ((src->fam_mask | src->put_mask[epoch]) & need) == need;
  }
  const ProjDev& hp = src->proj.host;                    // kernel.py:910-916, this side's share
  X.z_min[slot] = std::max(hp.w_z_min[0], hp.w_z_min[1]);
  X.z_max[slot] = std::min(hp.w_z_max[0], hp.w_z_max[1]);
  return CHOMP_OK;
}

int chomp_covariance_table_cross(chomp_ctx* ctx, double D_a, double D_b, double* ln_K,
                                 double* tables, double* levels, size_t n) {
  if (!ctx) return CHOMP_ERR_ARG;
  CrossState& X = ctx->cross;
  if (!X.staged[0] || !X.staged[1])
    return fail(ctx, CHOMP_ERR_STATE, "covariance_table_cross before covariance_cross_stage of both slots");
  if (X.which[0] == CHOMP_CROSS_WINDOWS || X.which[1] == CHOMP_CROSS_WINDOWS)
    return fail(ctx, CHOMP_ERR_STATE, "covariance_table_cross: a slot holds windows only (CHOMP_CROSS_WINDOWS)");
  if (!(D_a > 0.0) || !(D_b > 0.0)) return fail(ctx, CHOMP_ERR_ARG, "covariance_table_cross: D_a, D_b");
  const chomp_config& c = ctx->cfg;
  const ProjLayout L = make_proj_layout(c.cosmo_npoints, c.window_npoints, c.kernel_npoints);
  const CrossLayout& C = X.C;
  if (C.pd[0] - C.htab[0] != ctx->L.stride || C.N != L.NKT)
    return fail(ctx, CHOMP_ERR_STATE, "covariance_table_cross: the snapshots are of another configuration");
  if ((ln_K || tables || levels) && n != (size_t)C.N)
    return fail(ctx, CHOMP_ERR_ARG, "covariance_table_cross: length must be kernel_npoints");
  HIPCHK(hipSetDevice(ctx->device));
  X.ready = false;
  size_t sh;
  { const int rcl = cross_lds_bytes(ctx, L, "covariance_table_cross", &sh); if (rcl) return rcl; }
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_cov_cross_knots<BAO>, dim3((unsigned)C.N, 4), dim3(256), sh, ctx->stream,
                       c, ctx->L, L, C, X.which[0], X.which[1], D_a, D_b, X.d);
  });
  hipLaunchKernelGGL(k_cov_cross_spline, dim3(4), dim3(64), 0, ctx->stream, C, X.d);
  HIPCHK(hipGetLastError());
  X.ready = true;
  const size_t N = (size_t)C.N;
  return slab_read(ctx, X.d, {{ln_K, &C.ln_K, 1, N}, {tables, C.proj, 4, N}, {levels, C.lev, 4, N}});
}

int chomp_covariance_gaussian_cross(chomp_ctx* ctx, double j0_limit, double area,
                                    double poisson_0, double poisson_1, double poisson_2,
                                    double poisson_3, const double* theta, size_t n, double* out,
                                    int mem) {
  if (!ctx || !theta || !out || n == 0)
    return fail(ctx, CHOMP_ERR_ARG, "covariance_gaussian_cross: bad args");
  Staging st(ctx, mem, "covariance_gaussian_cross");
  if (st.rc) return st.rc;
  if (!ctx->cross.ready)
    return fail(ctx, CHOMP_ERR_STATE, "covariance_gaussian_cross before covariance_table_cross");
  int rc = gaussian_scalars(ctx, "covariance_gaussian_cross", j0_limit, area);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  rc = gaussian_theta(ctx, "covariance_gaussian_cross", st.host, theta, n);
  if (rc) return rc;
  const double* d_theta;
  double* d_out;
  st.in(theta, 2 * n, &d_theta);
  st.out(out, n, &d_out);
  rc = st.place();
  if (rc) return rc;
  const CrossLayout& C = ctx->cross.C;
  const size_t sh = gaussian_lds_bytes(C.N, 4);
  hipLaunchKernelGGL(k_cov_cross_gaussian, dim3((unsigned)n), dim3(256), sh, ctx->stream, ctx->cfg,
                     C, ctx->cross.d, ctx->d_j0, j0_limit, area, poisson_0, poisson_1, poisson_2,
                     poisson_3, d_theta, d_theta + n, d_out, (double*)nullptr);
  return st.finish();
}

// ---------------------------------------------------------------------------
// Every Gaussian block of a CovarianceMulti in one call (chomp_proj_kernels.h, "The block axis
// of the Gaussian covariance")
// ---------------------------------------------------------------------------
// Correlation c is projection set c of the last set-up of sets and P(k) epoch epoch[c] of this
// context; block (i, j) reads both sides where they lie.  Neither ctx->proj nor ctx->cross nor
// the single-block covariance state is touched.
int chomp_covariance_blocks(chomp_ctx* ctx, int which, size_t n_corr, const size_t* epoch,
                            double j0_limit, double area, const double* poisson,
                            const double* theta, size_t n_pairs, double* out, int mem) {
  StageRange range_(ctx, "chomp:covariance_blocks");
  if (!ctx) return CHOMP_ERR_ARG;
  BlocksCall A(ctx, "covariance_blocks", mem, n_corr, n_pairs);
  int rc = A.head(epoch && poisson && theta && out, false);
  if (rc) return rc;
  Staging& st = A.st;
  const ProjSets& S = A.S;
  const size_t n_blocks = A.n_blocks;
  if (n_pairs > 0x7fffffffu / n_blocks) return A.refuse(CHOMP_ERR_ARG, ": n_pairs * n_blocks too large");
  rc = A.epochs([&](size_t c) { return check_power(ctx, which, epoch[c], 1); });
  if (!rc) rc = gaussian_scalars(ctx, A.who, j0_limit, area);
  if (!rc) rc = gaussian_theta(ctx, A.who, st.host, theta, n_pairs);
  if (rc) return rc;
  const ProjLayout& L = A.L;
  const CrossLayout C = make_blocks_layout(L.NKT);
  size_t sh;
  rc = cross_lds_bytes(ctx, L, A.who, &sh);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  for (size_t c = 0; c < n_corr; ++c) {                  // (a no-op unless `which` extrapolates)
    const int rce = prepare_extrapolation(ctx, which, epoch[c], 1);
    if (rce) return rce;
  }
  BlocksState& B = ctx->blocks;
  B.n_corr = 0;
  rc = ensure(ctx, B.d, n_blocks * (size_t)C.total);
  if (!rc) rc = blocks_index_upload(ctx, B.d_index, blocks_index(n_corr, epoch, false));
  if (rc) return rc;
  const double *d_theta, *d_poisson;
  double* d_out;
  st.in(theta, 2 * n_pairs, &d_theta);
  st.in(poisson, 4 * n_blocks, &d_poisson);
  st.out(out, n_blocks * n_pairs, &d_out);
  rc = st.place();
  if (rc) return rc;
  B.C = C;
  const int nc = A.nc;
  const unsigned Z = A.Z;
  const size_t pstride = A.pstride;
  hipLaunchKernelGGL(k_cov_blocks_prep, dim3((Z + 63) / 64), dim3(64), 0, ctx->stream, L, C, nc,
                     (int)n_blocks, S.d_pd, S.d_tab, pstride, B.d_index, B.d);
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_cov_blocks_knots<BAO>, dim3((unsigned)C.N, 4, Z), dim3(256), sh,
                       ctx->stream, ctx->cfg, ctx->L, L, C, nc, ctx->d_epochs, ctx->d_tab, which,
                       S.d_pd, S.d_tab, pstride, B.d_index, B.d);
  });
  hipLaunchKernelGGL(k_cov_blocks_spline, dim3(4, Z), dim3(64), 0, ctx->stream, C, nc, B.d_index, B.d);
  const size_t shg = gaussian_lds_bytes(C.N, 4);
  hipLaunchKernelGGL(k_cov_blocks_gaussian, dim3((unsigned)n_pairs, Z), dim3(256), shg, ctx->stream,
                     ctx->cfg, C, nc, B.d_index, B.d, ctx->d_j0, j0_limit, area, d_poisson, d_theta,
                     d_theta + n_pairs, d_out);
  HIPCHK(hipGetLastError());
  B.n_corr = n_corr;
  return st.finish();
}

// The tables of one block of the last chomp_covariance_blocks (host arrays, any may be NULL).
int chomp_covariance_blocks_table(chomp_ctx* ctx, size_t block, double* ln_K, double* tables,
                                  double* levels, double* scalars, size_t n) {
  if (!ctx) return CHOMP_ERR_ARG;
  const BlocksState& B = ctx->blocks;
  if (B.n_corr == 0) return fail(ctx, CHOMP_ERR_STATE, "covariance_blocks_table before covariance_blocks");
  const size_t n_blocks = B.n_corr * (B.n_corr + 1) / 2;
  if (block >= n_blocks) return fail(ctx, CHOMP_ERR_ARG, "covariance_blocks_table: block");
  const CrossLayout& C = B.C;
  if ((ln_K || tables || levels) && n != (size_t)C.N)
    return fail(ctx, CHOMP_ERR_ARG, "covariance_blocks_table: length must be kernel_npoints");
  bool diagonal = false;
  for (size_t i = 0, b0 = 0; i < B.n_corr; b0 += B.n_corr - i, ++i) diagonal = diagonal || block == b0;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int rows = diagonal ? 1 : 4;                       // (a diagonal block has table 0 alone)
  for (double* t : {tables, levels})
    if (t) std::fill(t + (size_t)rows * C.N, t + (size_t)4 * C.N, 0.0);
  const size_t N = (size_t)C.N;
  return slab_read(ctx, B.d + block * (size_t)C.total,
                   {{ln_K, &C.ln_K, 1, N}, {tables, C.proj, rows, N}, {levels, C.lev, rows, N},
                    {scalars, &C.scal, 1, 8}}, true);
}

// ---------------------------------------------------------------------------
// Gaussian covariance of C_l: CovarianceFourier (chomp_cov_kernels.h)
// ---------------------------------------------------------------------------
int chomp_covariance_fourier_zbar(chomp_ctx* ctx, const double* z, size_t n_z, double* info) {
  if (!ctx || !z) return fail(ctx, CHOMP_ERR_ARG, "covariance_fourier_zbar: bad args");
  if (n_z < 1 || n_z > 256)
    return fail(ctx, CHOMP_ERR_ARG, "covariance_fourier_zbar: the z grid must hold 1..256 points");
  const chomp_config& c = ctx->cfg;
  if (c.corr_npoints < 4)
    return fail(ctx, CHOMP_ERR_ARG, "covariance_fourier_zbar: corr_npoints must be at least 4");
  const ProjLayout L = make_proj_layout(c.cosmo_npoints, c.window_npoints, c.kernel_npoints);
  { const int rcs = check_cross_slots(ctx, L, "covariance_fourier_zbar", false); if (rcs) return rcs; }
  HIPCHK(hipSetDevice(ctx->device));
  FourierState& S = ctx->fourier;
  S.zbar = S.ready = false;
  const CrossState& X = ctx->cross;
  {   // covariance.py:887-903: every pair needs a redshift range, before anything is launched
    ProjDev hp[2];
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < 2; ++s)
      HIPCHK(hipMemcpy(&hp[s], X.d + X.C.pd[s], sizeof(ProjDev), hipMemcpyDeviceToHost));
    static const char* const names[4] = {"a1a2", "b1b2", "a1b2", "b1a2"};
    for (int p = 0; p < 4; ++p) {
      const ProjDev& p1 = hp[(p == kCovfB1B2 || p == kCovfB1A2) ? 1 : 0];
      const ProjDev& p2 = hp[(p == kCovfB1B2 || p == kCovfA1B2) ? 1 : 0];
      if (!(std::max(p1.w_z_min[0], p2.w_z_min[1]) < std::min(p1.w_z_max[0], p2.w_z_max[1])))
        return fail(ctx, CHOMP_ERR_SCOPE, std::string("covariance_fourier_zbar: the windows of "
                    "pair ") + names[p] + " have no redshift in common");
    }
  }
  const FourierLayout F = make_fourier_layout(c.corr_npoints);
  { const int rce = ensure(ctx, S.d, (size_t)F.total); if (rce) return rce; }
  S.F = F;
  Staging st(ctx, CHOMP_HOST, "covariance_fourier_zbar");
  const double* d_z;
  st.in(z, n_z, &d_z);
  const int rc = st.place();
  if (rc) return rc;
  hipLaunchKernelGGL(k_covf_zbar, dim3(4), dim3(256), 0, ctx->stream, L, F, cov_src(ctx, true), d_z,
                     (int)n_z, S.d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  S.zbar = true;
  if (info) {
    double sc[32];
    HIPCHK(hipMemcpy(sc, S.d + F.scal, sizeof(sc), hipMemcpyDeviceToHost));
    for (int p = 0; p < 4; ++p)
      for (int q = 0; q < 7; ++q) info[7 * p + q] = sc[8 * p + q];
  }
  return CHOMP_OK;
}

int chomp_covariance_fourier_table(chomp_ctx* ctx, int which, const size_t epoch[4],
                                   const double* ln_l, size_t n, double* norms, double* tables,
                                   double* levels) {
  if (!ctx || !epoch || !ln_l) return fail(ctx, CHOMP_ERR_ARG, "covariance_fourier_table: bad args");
  FourierState& S = ctx->fourier;
  if (!S.zbar) return fail(ctx, CHOMP_ERR_STATE, "covariance_fourier_table before covariance_fourier_zbar");
  if ((which & 15) != CHOMP_P_MM || (which & CHOMP_P_HALOFIT))
    return fail(ctx, CHOMP_ERR_SCOPE, "covariance_fourier_table: the tables are built from Halo.power_mm "
                                      "(CHOMP_P_MM, with or without CHOMP_P_EXTRAPOLATE)");
  for (int p = 0; p < 4; ++p) {
    const int rcp = check_power(ctx, which, epoch[p], 1);
    if (rcp) return rcp;
  }
  const chomp_config& c = ctx->cfg;
  const FourierLayout& F = S.F;
  if (n != (size_t)F.N || F.N != c.corr_npoints)
    return fail(ctx, CHOMP_ERR_ARG, "covariance_fourier_table: length must be corr_npoints");
  for (size_t i = 1; i < n; ++i)
    if (!(ln_l[i] > ln_l[i - 1]))
      return fail(ctx, CHOMP_ERR_ARG, "covariance_fourier_table: ln l knots must increase");
  const ProjLayout L = make_proj_layout(c.cosmo_npoints, c.window_npoints, c.kernel_npoints);
  { const int rcs = check_cross_slots(ctx, L, "covariance_fourier_table", false); if (rcs) return rcs; }
  HIPCHK(hipSetDevice(ctx->device));
  const size_t sh = (size_t)covf_lds_doubles(ctx->L.NK, L) * sizeof(double);
  if (!fits_lds(ctx->with_bao, &k_covf_knots<true>, &k_covf_knots<false>, sh))
    return fail(ctx, CHOMP_ERR_ARG, "covariance_fourier_table: halo/cosmo/window_npoints too large "
                                    "for the spectrum and the windows of a pair");
  S.ready = false;
  for (int p = 0; p < 4; ++p) {
    bool seen = false;
    for (int q = 0; q < p; ++q) seen = seen || epoch[q] == epoch[p];
    if (seen) continue;
    const int rce = prepare_extrapolation(ctx, which, epoch[p], 1);
    if (rce) return rce;
  }
  HIPCHK(hipMemcpyAsync(S.d + F.ln_l, ln_l, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_covf_knots<BAO>, dim3((unsigned)F.N, 4), dim3(256), sh, ctx->stream, c,
                       ctx->L, L, F, cov_src(ctx, true), ctx->d_epochs, ctx->d_tab, which,
                       (int)epoch[0], (int)epoch[1], (int)epoch[2], (int)epoch[3], S.d);
  });
  hipLaunchKernelGGL(k_covf_spline, dim3(4), dim3(64), 0, ctx->stream, F, S.d);
  HIPCHK(hipGetLastError());
  // (the copy above reads the caller's array: done before the call returns)
  HIPCHK(hipStreamSynchronize(ctx->stream));
  S.ln_l_min = ln_l[0];
  S.ln_l_max = ln_l[n - 1];
  S.ready = true;
  const size_t b = (size_t)F.N * sizeof(double);
  for (int p = 0; p < 4; ++p) {
    if (norms) HIPCHK(hipMemcpy(norms + p, S.d + F.scal + 8 * p + kCovfNorm, sizeof(double), hipMemcpyDeviceToHost));
    if (tables) HIPCHK(hipMemcpy(tables + (size_t)p * F.N, S.d + F.tab[p], b, hipMemcpyDeviceToHost));
    if (levels) HIPCHK(hipMemcpy(levels + (size_t)p * F.N, S.d + F.lev[p], b, hipMemcpyDeviceToHost));
  }
  return CHOMP_OK;
}

int chomp_covariance_fourier_gaussian(chomp_ctx* ctx, const double* l, size_t n, double* out,
                                      int mem) {
  if (!ctx || !l || !out || n == 0)
    return fail(ctx, CHOMP_ERR_ARG, "covariance_fourier_gaussian: bad args");
  Staging st(ctx, mem, "covariance_fourier_gaussian");
  if (st.rc) return st.rc;
  const FourierState& S = ctx->fourier;
  if (!S.ready)
    return fail(ctx, CHOMP_ERR_STATE, "covariance_fourier_gaussian before covariance_fourier_table");
  HIPCHK(hipSetDevice(ctx->device));
  const double* d_l;
  double* d_out;
  st.in(l, 2 * n, &d_l);
  st.out(out, 5 * n, &d_out);
  const int rc = st.place();
  if (rc) return rc;
  hipLaunchKernelGGL(k_covf_eval, grid_1d(n), dim3(256), 0, ctx->stream, S.F, S.d, S.ln_l_min,
                     S.ln_l_max, d_l, n, d_out);
  return st.finish();
}

// ---------------------------------------------------------------------------
// Super-sample covariance of w(theta) (chomp_cov_kernels.h)
// ---------------------------------------------------------------------------
// The plan of the context's kernel_ssc state (set by kernel_ssc_setup).
static SscPlan ssc_plan_of(const chomp_ctx* ctx) {
  return ssc_plan(ctx->cfg, ctx->L.NK, ctx->proj.L, ctx->proj.ssc_ns);
}

static int kernel_ssc_setup(chomp_ctx* ctx, bool four, double ln_ktheta_min, double ln_ktheta_max,
                            double j0_ssc_limit, const double* ln_chi, const double* sigma2,
                            size_t n_sigma, int with_table, double* info, double* table,
                            double* levels) {
  if (!ctx || !ln_chi || !sigma2) return fail(ctx, CHOMP_ERR_ARG, "kernel_ssc_setup: bad args");
  if (!with_table && (table || levels))
    return fail(ctx, CHOMP_ERR_ARG, "kernel_ssc_setup: table / levels need with_table");
  if (!ctx->proj.ready) return fail(ctx, CHOMP_ERR_STATE, "kernel_ssc_setup before kernel_setup");
  if (!(ln_ktheta_max > ln_ktheta_min) || !(j0_ssc_limit > 0.0))
    return fail(ctx, CHOMP_ERR_ARG, "kernel_ssc_setup: ln(k theta) range / J0 limit");
  const int N = ctx->proj.L.NKT;
  if (n_sigma < 4 || n_sigma > 256 || N < 4 || N > 256)
    return fail(ctx, CHOMP_ERR_ARG, "kernel_ssc_setup: corr_npoints and kernel_npoints must be "
                                    "4..256");
  for (size_t i = 1; i < n_sigma; ++i)
    if (!(ln_chi[i] > ln_chi[i - 1]))
      return fail(ctx, CHOMP_ERR_ARG, "kernel_ssc_setup: ln chi knots must increase");
  ProjState& P = ctx->proj;
  const ProjLayout& L = P.L;
  if (four) { const int rcx = check_cross_slots(ctx, L, "kernel_ssc_setup_cross", true); if (rcx) return rcx; }
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  const SscPlan plan = ssc_plan(ctx->cfg, ctx->L.NK, L, (int)n_sigma);
  const SscLayout& S = plan.S;
  const size_t sh = plan.sh_table[four];
  if (four && !fits_lds(&k_ssc_table<true>, sh))
    return fail(ctx, CHOMP_ERR_ARG, "kernel_ssc_setup_cross: cosmo/window/corr_npoints too large "
                                    "for the four windows of a cross block");
  P.ssc_ready = false;
  P.ssc_prep = false;
  { const int rce = ensure(ctx, P.d_ssc, (size_t)S.total); if (rce) return rce; }
  HIPCHK(hipMemcpyAsync(P.d_ssc + S.sx, ln_chi, n_sigma * sizeof(double), hipMemcpyHostToDevice,
                        ctx->stream));
  HIPCHK(hipMemcpyAsync(P.d_ssc + S.sy, sigma2, n_sigma * sizeof(double), hipMemcpyHostToDevice,
                        ctx->stream));
  const CovSrc src = cov_src(ctx, four);
  with_flag(four, [&](auto FOUR) {
    hipLaunchKernelGGL(k_ssc_prep<FOUR>, dim3(1), dim3(256), 0, ctx->stream, ctx->cfg, L, S, src,
                       ln_ktheta_min, ln_ktheta_max, j0_ssc_limit, P.d_ssc);
    if (with_table)
      hipLaunchKernelGGL(k_ssc_table<FOUR>, dim3(plan.n_tab), dim3(256), sh,
                         ctx->stream, ctx->cfg, L, S, src, ctx->d_j0, P.d_ssc,
                         (const double*)nullptr, (const double*)nullptr, (double*)nullptr);
  });
  if (with_table)
    hipLaunchKernelGGL(k_ssc_bicubic, dim3(1), dim3(256), 0, ctx->stream, S, P.d_ssc);
  HIPCHK(hipGetLastError());
  P.ssc_ns = (int)n_sigma;
  P.ssc_four = four;
  P.ssc_prep = true;
  P.ssc_ready = with_table != 0;
  const size_t NN = (size_t)N * N;
  return slab_read(ctx, P.d_ssc, {{info, &S.scal, 1, 3}, {table, &S.tab, 1, NN}, {levels, &S.lev, 1, NN}});
}

int chomp_kernel_ssc_setup(chomp_ctx* ctx, double ln_ktheta_min, double ln_ktheta_max,
                           double j0_ssc_limit, const double* ln_chi, const double* sigma2,
                           size_t n_sigma, int with_table, double* info, double* table,
                           double* levels) {
  return kernel_ssc_setup(ctx, false, ln_ktheta_min, ln_ktheta_max, j0_ssc_limit, ln_chi, sigma2,
                          n_sigma, with_table, info, table, levels);
}

int chomp_kernel_ssc_setup_cross(chomp_ctx* ctx, double ln_ktheta_min, double ln_ktheta_max,
                                 double j0_ssc_limit, const double* ln_chi, const double* sigma2,
                                 size_t n_sigma, int with_table, double* info, double* table,
                                 double* levels) {
  return kernel_ssc_setup(ctx, true, ln_ktheta_min, ln_ktheta_max, j0_ssc_limit, ln_chi, sigma2,
                          n_sigma, with_table, info, table, levels);
}

int chomp_covariance_cross_range(chomp_ctx* ctx, double* info) {
  if (!ctx || !info) return fail(ctx, CHOMP_ERR_ARG, "covariance_cross_range: bad args");
  if (!ctx->proj.ready) return fail(ctx, CHOMP_ERR_STATE, "covariance_cross_range before kernel_setup");
  { const int rcx = check_cross_slots(ctx, ctx->proj.L, "covariance_cross_range", true); if (rcx) return rcx; }
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  Staging st(ctx, CHOMP_HOST, "covariance_cross_range");
  double* d_out;
  st.out(info, 4, &d_out);
  const int rc = st.place();
  if (rc) return rc;
  hipLaunchKernelGGL(k_cov_cross_range, dim3(1), dim3(64), 0, ctx->stream, ctx->cfg, ctx->proj.L,
                     cov_src(ctx, true), d_out);
  return st.finish();
}

int chomp_kernel_ssc_raw(chomp_ctx* ctx, const double* ln_ktheta, size_t n, double* out) {
  return pair_eval(ctx, "kernel_ssc_raw", "kernel_ssc_setup", &ProjState::ssc_prep, 0, true, ln_ktheta,
                   n, out, [&](const double* d_in, double* d_out) {
    const ProjState& P = ctx->proj;
    const SscPlan plan = ssc_plan_of(ctx);
    const CovSrc src = cov_src(ctx, P.ssc_four);
    with_flag(P.ssc_four, [&](auto FOUR) {
      hipLaunchKernelGGL(k_ssc_table<FOUR>, dim3((unsigned)n), dim3(256), plan.sh_table[P.ssc_four],
                         ctx->stream, ctx->cfg, P.L, plan.S, src, ctx->d_j0, P.d_ssc, d_in, d_in + n,
                         d_out);
    });
  });
}

int chomp_kernel_ssc_eval(chomp_ctx* ctx, const double* ln_ktheta, size_t n, double* out) {
  return pair_eval(ctx, "kernel_ssc_eval", "kernel_ssc_setup", &ProjState::ssc_ready, 0, false,
                   ln_ktheta, n, out, [&](const double* d_in, double* d_out) {
    const ProjState& P = ctx->proj;
    hipLaunchKernelGGL(k_ssc_eval, grid_1d(n), dim3(256), 0, ctx->stream,
                       make_ssc_layout(P.L.NKT, P.ssc_ns), P.d_ssc, d_in, d_in + n, (int)n, d_out);
  });
}

int chomp_covariance_ssc(chomp_ctx* ctx, size_t epoch, double area, const double* theta,
                         size_t n, double* out, double* kb_knots, double* kb_levels) {
  if (!ctx || !theta || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "covariance_ssc: bad args");
  if (!ctx->proj.ready || !ctx->proj.ssc_ready)
    return fail(ctx, CHOMP_ERR_STATE, "covariance_ssc before kernel_ssc_setup");
  if (ctx->proj.ssc_four)
    return fail(ctx, CHOMP_ERR_STATE, "covariance_ssc: the kernel_ssc table is a cross block's "
                                      "(chomp_covariance_ssc_cross serves it)");
  int rc = pairs_check(ctx, "covariance_ssc", area, n);
  if (!rc) rc = check_power(ctx, CHOMP_P_SSC_RESPONSE, epoch, 1, true);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  const ProjState& P = ctx->proj;
  const SscPlan plan = ssc_plan_of(ctx);
  rc = pairs_positive(ctx, "covariance_ssc", theta, n);
  if (rc) return rc;
  Staging st(ctx, CHOMP_HOST, "covariance_ssc");
  PairArrays d;
  d.stage(st, theta, n, plan.NK, out, kb_knots, kb_levels);
  rc = st.place();
  if (rc) return rc;
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_ssc_kb<BAO>, dim3((unsigned)plan.NK, (unsigned)n), dim3(256), plan.sh_kb[0],
                       ctx->stream, ctx->cfg, ctx->L, plan.S, ctx->d_epochs, (int)epoch, ctx->d_tab,
                       P.d_ssc, d.theta, d.theta + n, d.knots, d.lev);
  });
  return pairs_finish(ctx, st, d, n, plan.sh_outer, area);
}

int chomp_covariance_ssc_cross(chomp_ctx* ctx, double area, const double* theta, size_t n,
                               double* out, double* kb_knots, double* kb_levels) {
  if (!ctx || !theta || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "covariance_ssc_cross: bad args");
  if (!ctx->proj.ready || !ctx->proj.ssc_ready || !ctx->proj.ssc_four)
    return fail(ctx, CHOMP_ERR_STATE, "covariance_ssc_cross before kernel_ssc_setup_cross");
  const ProjState& P = ctx->proj;
  { const int rcx = check_cross_slots(ctx, P.L, "covariance_ssc_cross", true); if (rcx) return rcx; }
  const CrossState& X = ctx->cross;
  if (!X.response[0] || !X.response[1])
    return fail(ctx, CHOMP_ERR_STATE, "covariance_ssc_cross: the staged epochs do not hold the "
                                      "knot tables of the super-sample response (h_m, pp_mm, i_1_2)");
  int rc = pairs_check(ctx, "covariance_ssc_cross", area, n);
  if (!rc) rc = pairs_positive(ctx, "covariance_ssc_cross", theta, n);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  const SscPlan plan = ssc_plan_of(ctx);
  if (!fits_lds(ctx->with_bao, &k_ssc_kb_cross<true>, &k_ssc_kb_cross<false>, plan.sh_kb[1]))
    return fail(ctx, CHOMP_ERR_ARG, "covariance_ssc_cross: halo/kernel_npoints too large for the "
                                    "two responses of a cross block");
  Staging st(ctx, CHOMP_HOST, "covariance_ssc_cross");
  PairArrays d;
  d.stage(st, theta, n, plan.NK, out, kb_knots, kb_levels);
  rc = st.place();
  if (rc) return rc;
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_ssc_kb_cross<BAO>, dim3((unsigned)plan.NK, (unsigned)n), dim3(256),
                       plan.sh_kb[1], ctx->stream, ctx->cfg, ctx->L, plan.S, X.C, X.d, P.d_ssc,
                       d.theta, d.theta + n, d.knots, d.lev);
  });
  return pairs_finish(ctx, st, d, n, plan.sh_outer, area);
}

// ---------------------------------------------------------------------------
// The super-sample term of every block of a CovarianceMulti in one call (chomp_cov_kernels.h,
// "The block axis of the super-sample term")
// ---------------------------------------------------------------------------
int chomp_covariance_ssc_blocks_range(chomp_ctx* ctx, size_t n_corr, double* info) {
  if (!ctx) return CHOMP_ERR_ARG;
  if (!info || n_corr == 0) return fail(ctx, CHOMP_ERR_ARG, "covariance_ssc_blocks_range: bad args");
  int rc = blocks_check(ctx, "covariance_ssc_blocks_range", n_corr, true);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  const ProjSets& S = ctx->sets;
  const size_t n_blocks = n_corr * (n_corr + 1) / 2;
  // (the index block of the super-sample calls, in their state's buffer)
  rc = blocks_index_upload(ctx, ctx->ssc_blocks.d_index, blocks_index(n_corr, nullptr, true));
  if (rc) return rc;
  Staging st(ctx, CHOMP_HOST, "covariance_ssc_blocks_range");
  double* d_out;
  st.out(info, 4 * n_blocks, &d_out);
  rc = st.place();
  if (rc) return rc;
  hipLaunchKernelGGL(k_ssc_blocks_range, dim3((unsigned)((n_blocks + 63) / 64)), dim3(64), 0,
                     ctx->stream, ctx->cfg, S.L, (int)n_corr, (int)n_blocks, S.d_pd, S.d_tab,
                     (size_t)S.L.total, ctx->ssc_blocks.d_index, d_out);
  return st.finish();
}

// Correlation c is projection set c of the last set-up of sets and halo epoch epoch[c] of this
// context; block (i, j) reads both sides where they lie.  Neither ctx->proj (d_ssc included) nor
// ctx->cross nor the state of chomp_covariance_blocks is touched.
int chomp_covariance_ssc_blocks(chomp_ctx* ctx, size_t n_corr, const size_t* epoch,
                                double ln_ktheta_min, double ln_ktheta_max, double j0_ssc_limit,
                                const double* ln_chi, const double* sigma2, size_t n_sigma,
                                double area, const double* theta, size_t n_pairs, double* out,
                                int mem) {
  StageRange range_(ctx, "chomp:covariance_ssc_blocks");
  if (!ctx) return CHOMP_ERR_ARG;
  BlocksCall A(ctx, "covariance_ssc_blocks", mem, n_corr, n_pairs);
  int rc = A.head(epoch && ln_chi && sigma2 && theta && out, true);
  if (!rc) rc = A.epochs([&](size_t c) { return check_power(ctx, CHOMP_P_SSC_RESPONSE, epoch[c], 1, true); });
  if (rc) return rc;
  const ProjLayout& L = A.L;
  const size_t n_blocks = A.n_blocks;
  if (!(ln_ktheta_max > ln_ktheta_min) || !(j0_ssc_limit > 0.0))
    return A.refuse(CHOMP_ERR_ARG, ": ln(k theta) range / J0 limit");
  if (n_sigma < 4 || n_sigma > 256 || L.NKT < 4 || L.NKT > 256)
    return A.refuse(CHOMP_ERR_ARG, ": corr_npoints and kernel_npoints must be 4..256");
  for (size_t b = 0; b < n_blocks; ++b)
    for (size_t q = 1; q < n_sigma; ++q)
      if (!(ln_chi[b * n_sigma + q] > ln_chi[b * n_sigma + q - 1]))
        return A.refuse(CHOMP_ERR_ARG, ": block " + std::to_string(b) + ": ln chi knots must increase");
  rc = pairs_check(ctx, A.who, area, n_pairs);
  if (!rc) rc = gaussian_theta(ctx, A.who, A.st.host, theta, n_pairs);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  const SscPlan plan = ssc_plan(ctx->cfg, ctx->L.NK, L, (int)n_sigma);
  const SscLayout& S = plan.S;
  const int NK = plan.NK;
  if (!fits_lds(&k_ssc_blocks_table<false>, plan.sh_table[0]) ||
      (A.n_cross && !fits_lds(&k_ssc_blocks_table<true>, plan.sh_table[1])))
    return A.refuse(CHOMP_ERR_ARG, ": cosmo/window/corr_npoints too large for the windows of a block");
  // (one kernel runs both k_b bodies: the launch takes the LDS of the larger)
  if (!fits_lds(ctx->with_bao, &k_ssc_blocks_kb<true>, &k_ssc_blocks_kb<false>, plan.sh_kb[1]))
    return A.refuse(CHOMP_ERR_ARG, ": halo/kernel_npoints too large for the two responses of a cross block");
  SscBlocksState& B = ctx->ssc_blocks;
  rc = A.begin(B, n_blocks * (size_t)S.total, 2 * n_blocks * n_pairs * (size_t)NK, epoch);
  if (!rc) rc = ensure(ctx, B.d_sigma, 2 * n_blocks * n_sigma);
  if (rc) return rc;
  double* d_ln_chi = B.d_sigma;
  double* d_sigma2 = d_ln_chi + n_blocks * n_sigma;
  HIPCHK(hipMemcpyAsync(d_ln_chi, ln_chi, n_blocks * n_sigma * sizeof(double), hipMemcpyHostToDevice,
                        ctx->stream));
  HIPCHK(hipMemcpyAsync(d_sigma2, sigma2, n_blocks * n_sigma * sizeof(double), hipMemcpyHostToDevice,
                        ctx->stream));
  rc = A.place(theta, out);
  if (rc) return rc;
  B.S = S;
  A.lists(&k_ssc_blocks_prep<false>, &k_ssc_blocks_prep<true>, 0, {0, 0}, S, ln_ktheta_min,
          ln_ktheta_max, j0_ssc_limit, d_ln_chi, d_sigma2, B.d);
  A.lists(&k_ssc_blocks_table<false>, &k_ssc_blocks_table<true>, plan.n_tab, plan.sh_table, S,
          ctx->d_j0, B.d);
  hipLaunchKernelGGL(k_ssc_blocks_bicubic, dim3(A.Z), dim3(256), 0, ctx->stream, S, B.d);
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_ssc_blocks_kb<BAO>, dim3((unsigned)NK, (unsigned)n_pairs, A.Z), dim3(256),
                       plan.sh_kb[1], ctx->stream, ctx->cfg, ctx->L, S, A.nc, ctx->d_epochs, ctx->d_tab,
                       A.d_index, B.d, A.d_theta, A.d_theta + n_pairs, A.d_knots, A.d_lev);
  });
  return A.finish(B, plan.sh_outer, area);
}

// One block of the last chomp_covariance_ssc_blocks (host arrays, any may be NULL).
int chomp_covariance_ssc_blocks_table(chomp_ctx* ctx, size_t block, double* info, double* table,
                                      double* levels, double* kb_knots, double* kb_levels) {
  if (!ctx) return CHOMP_ERR_ARG;
  const SscBlocksState& B = ctx->ssc_blocks;
  return term_blocks_table(ctx, "covariance_ssc_blocks", B, B.S, block, info, table, levels, nullptr,
                           0, kb_knots, kb_levels);
}

// ---------------------------------------------------------------------------
// One-halo trispectrum term of the covariance of w(theta) (chomp_cov_kernels.h)
// ---------------------------------------------------------------------------
// The status word CHOMP_ST_COV_NG_DIVMAX goes to: the context's first epoch, if it has one.
static unsigned* ng_status(chomp_ctx* ctx) {
  return ctx->n_epoch > 0 ? ctx->d_status : nullptr;
}

int chomp_kernel_ng_setup(chomp_ctx* ctx, double j0_limit, int with_table, double* table,
                          double* levels, double* table_min) {
  if (!ctx) return fail(ctx, CHOMP_ERR_ARG, "kernel_ng_setup: bad args");
  if (!with_table && (table || levels || table_min))
    return fail(ctx, CHOMP_ERR_ARG, "kernel_ng_setup: table / levels / min need with_table");
  if (!ctx->proj.ready || !ctx->proj.ssc_prep)
    return fail(ctx, CHOMP_ERR_STATE, "kernel_ng_setup before kernel_ssc_setup");
  if (!(j0_limit > 0.0)) return fail(ctx, CHOMP_ERR_ARG, "kernel_ng_setup: J0 limit");
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  ProjState& P = ctx->proj;
  const ProjLayout& L = P.L;
  const SscLayout S = make_ssc_layout(L.NKT, P.ssc_ns);
  const NgPlan plan = ng_plan(ctx->cfg, L);
  const NgLayout& G = plan.G;
  // (the windows are those of the kernel_ssc state: a cross block's four, or the context's two)
  const bool four = P.ssc_four;
  if (four) { const int rcx = check_cross_slots(ctx, L, "kernel_ng_setup", true); if (rcx) return rcx; }
  const size_t sh = plan.sh_table[four];
  if (four && !fits_lds(&k_ng_table<true>, sh))
    return fail(ctx, CHOMP_ERR_ARG, "kernel_ng_setup: cosmo/window_npoints too large for the four "
                                    "windows of a cross block");
  P.ng_ready = false;
  P.ng_prep = false;
  { const int rce = ensure(ctx, P.d_ng, (size_t)G.total); if (rce) return rce; }
  hipLaunchKernelGGL(k_ng_prep, dim3(1), dim3(256), 0, ctx->stream, S, G, P.d_ssc, j0_limit,
                     P.d_ng, ng_status(ctx));
  if (with_table) {
    const CovSrc src = cov_src(ctx, four);
    with_flag(four, [&](auto FOUR) {
      hipLaunchKernelGGL(k_ng_table<FOUR>, dim3(plan.n_tab), dim3(256), sh,
                         ctx->stream, ctx->cfg, L, G, src, ctx->d_j0, P.d_ng,
                         (const double*)nullptr, (const double*)nullptr, (double*)nullptr,
                         ng_status(ctx));
    });
    hipLaunchKernelGGL(k_ng_bicubic, dim3(1), dim3(256), 0, ctx->stream, G, P.d_ng);
  }
  HIPCHK(hipGetLastError());
  P.ng_four = four;
  P.ng_prep = true;
  P.ng_ready = with_table != 0;
  const int at_min = G.scal + kNgMin;
  const size_t NN = (size_t)G.N * G.N;
  return slab_read(ctx, P.d_ng, {{table, &G.tab, 1, NN}, {levels, &G.lev, 1, NN}, {table_min, &at_min, 1, 1}});
}

int chomp_kernel_ng_raw(chomp_ctx* ctx, const double* ln_ktheta, size_t n, double* out) {
  return pair_eval(ctx, "kernel_ng_raw", "kernel_ng_setup", &ProjState::ng_prep, (size_t)INT32_MAX, true,
                   ln_ktheta, n, out, [&](const double* d_in, double* d_out) {
    const ProjState& P = ctx->proj;
    const NgPlan plan = ng_plan(ctx->cfg, P.L);
    const CovSrc src = cov_src(ctx, P.ng_four);
    with_flag(P.ng_four, [&](auto FOUR) {
      hipLaunchKernelGGL(k_ng_table<FOUR>, dim3((unsigned)n), dim3(256), plan.sh_table[P.ng_four],
                         ctx->stream, ctx->cfg, P.L, plan.G, src, ctx->d_j0, P.d_ng, d_in, d_in + n,
                         d_out, ng_status(ctx));
    });
  });
}

int chomp_kernel_ng_eval(chomp_ctx* ctx, const double* ln_ktheta, size_t n, double* out) {
  return pair_eval(ctx, "kernel_ng_eval", "kernel_ng_setup", &ProjState::ng_ready, (size_t)INT32_MAX,
                   false, ln_ktheta, n, out, [&](const double* d_in, double* d_out) {
    const ProjState& P = ctx->proj;
    hipLaunchKernelGGL(k_ng_eval, grid_1d(n), dim3(256), 0, ctx->stream, make_ng_layout(P.L.NKT),
                       P.d_ng, d_in, d_in + n, (int)n, d_out);
  });
}

int chomp_covariance_ng(chomp_ctx* ctx, double area, const double* tri_table, size_t n_tri,
                        double tri_k_min, double tri_k_max, const double* theta, size_t n,
                        double* out, double* kb_knots, double* kb_levels) {
  if (!ctx || !tri_table || !theta || !out || n == 0)
    return fail(ctx, CHOMP_ERR_ARG, "covariance_ng: bad args");
  if (!ctx->proj.ready || !ctx->proj.ng_ready)
    return fail(ctx, CHOMP_ERR_STATE, "covariance_ng before kernel_ng_setup");
  int rc = pairs_check(ctx, "covariance_ng", area, n);
  if (rc) return rc;
  if (n_tri < 4 || n_tri > 64)
    return fail(ctx, CHOMP_ERR_ARG, "covariance_ng: the I_0^4 table must be 4..64 knots a side");
  if (!(tri_k_min > 0.0) || !(tri_k_max > tri_k_min))
    return fail(ctx, CHOMP_ERR_ARG, "covariance_ng: the I_0^4 table's k range");
  rc = pairs_positive(ctx, "covariance_ng", theta, n);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  ProjState& P = ctx->proj;
  const NgPlan plan = ng_plan(ctx->cfg, P.L);
  const NgLayout& G = plan.G;
  const NgTriLayout T = make_ng_tri_layout((int)n_tri);
  { const int rce = ensure(ctx, P.d_ng_tri, (size_t)T.total); if (rce) return rce; }
  Staging st(ctx, CHOMP_HOST, "covariance_ng");
  PairArrays d;
  const double* d_tri_in;
  d.stage(st, theta, n, plan.NK, out, kb_knots, kb_levels);
  st.in(tri_table, n_tri * n_tri, &d_tri_in);
  rc = st.place();
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(P.d_ng_tri + T.tab, d_tri_in, n_tri * n_tri * sizeof(double),
                        hipMemcpyDeviceToDevice, ctx->stream));
  hipLaunchKernelGGL(k_ng_tri, dim3(1), dim3(256), 0, ctx->stream, T, tri_k_min, tri_k_max,
                     P.d_ng_tri);
  const size_t sh = (size_t)ng_kb_lds_doubles(G.N, T.N) * sizeof(double);
  hipLaunchKernelGGL(k_ng_kb, dim3((unsigned)plan.NK, (unsigned)n), dim3(256), sh, ctx->stream,
                     ctx->cfg, G, T, P.d_ng, P.d_ng_tri, tri_k_min, tri_k_max, d.theta, d.theta + n,
                     d.knots, d.lev, ng_status(ctx));
  return pairs_finish(ctx, st, d, n, plan.sh_outer, area);
}

// ---------------------------------------------------------------------------
// The trispectrum term of every block of a CovarianceMulti in one call (chomp_cov_kernels.h,
// "The block axis of the trispectrum term")
// ---------------------------------------------------------------------------
// Correlation c is projection set c of the last set-up of sets; block (i, j) reads both sides
// where they lie, and epoch[c] only names a status word.  Neither ctx->proj (d_ssc, d_ng and
// d_ng_tri included) nor ctx->cross nor the states of chomp_covariance_blocks and
// chomp_covariance_ssc_blocks are touched.
//
// What a call of n_corr correlations and n_pairs pairs of angles keeps on the device, in elements:
// the slabs (n_blocks NgLayout blocks of n_ktheta knots a side), the k_b buffer (knots, then
// levels), the I_0^4 block and the index block.  Host arithmetic alone.
struct NgBlocksSizes {
  size_t n_blocks, slab, slabs, kb, tri, index;
};
static NgBlocksSizes ng_blocks_sizes(size_t n_corr, size_t n_pairs, int n_ktheta, int n_k, int n_tri) {
  NgBlocksSizes Z;
  Z.n_blocks = n_corr * (n_corr + 1) / 2;
  Z.slab = (size_t)make_ng_layout(n_ktheta).total;
  Z.slabs = Z.n_blocks * Z.slab;
  Z.kb = 2 * Z.n_blocks * n_pairs * (size_t)n_k;
  Z.tri = (size_t)make_ng_tri_layout(n_tri).total;
  Z.index = n_corr + 3 * Z.n_blocks;
  return Z;
}

int chomp_covariance_ng_blocks_plan(size_t n_corr, const size_t* epoch, size_t n_pairs,
                                    size_t n_ktheta, size_t n_k, size_t n_tri, size_t* sizes,
                                    int* index) {
  if (!sizes || n_corr == 0 || n_corr > (size_t)kProjSetsMax || n_corr * (n_corr + 1) / 2 > 65535 ||
      n_pairs == 0 || n_pairs > 65535 ||
      n_ktheta < 4 || n_ktheta > 256 || n_k < 4 || n_k > 256 || n_tri < 4 || n_tri > 64)
    return CHOMP_ERR_ARG;
  const NgBlocksSizes Z = ng_blocks_sizes(n_corr, n_pairs, (int)n_ktheta, (int)n_k, (int)n_tri);
  const size_t out[6] = {Z.n_blocks, Z.slab, Z.slabs, Z.kb, Z.tri, Z.index};
  std::copy(out, out + 6, sizes);
  if (index) {
    const std::vector<int> block = blocks_index(n_corr, epoch, true);
    std::copy(block.begin(), block.end(), index);
  }
  return CHOMP_OK;
}

int chomp_covariance_ng_blocks(chomp_ctx* ctx, size_t n_corr, const size_t* epoch,
                               double ln_ktheta_min, double ln_ktheta_max, double j0_limit,
                               double area, const double* tri_table, size_t n_tri,
                               double tri_k_min, double tri_k_max, const double* theta,
                               size_t n_pairs, double* out, int mem) {
  StageRange range_(ctx, "chomp:covariance_ng_blocks");
  if (!ctx) return CHOMP_ERR_ARG;
  BlocksCall A(ctx, "covariance_ng_blocks", mem, n_corr, n_pairs);
  // (with `overlap`: a block whose windows share no redshift is refused here, from the host's
  //  ranges of the sets)
  int rc = A.head(tri_table && theta && out, true);
  if (!rc && epoch)
    rc = A.epochs([&](size_t c) {
      return epoch[c] >= ctx->n_epoch ? fail(ctx, CHOMP_ERR_ARG, "epoch range") : CHOMP_OK;
    });
  if (rc) return rc;
  const ProjLayout& L = A.L;
  if (!(ln_ktheta_max > ln_ktheta_min) || !(j0_limit > 0.0))
    return A.refuse(CHOMP_ERR_ARG, ": ln(k theta) range / J0 limit");
  if (L.NKT < 4 || L.NKT > 256) return A.refuse(CHOMP_ERR_ARG, ": kernel_npoints must be 4..256");
  rc = pairs_check(ctx, A.who, area, n_pairs);
  if (rc) return rc;
  if (n_tri < 4 || n_tri > 64)
    return A.refuse(CHOMP_ERR_ARG, ": the I_0^4 table must be 4..64 knots a side");
  if (!(tri_k_min > 0.0) || !(tri_k_max > tri_k_min))
    return A.refuse(CHOMP_ERR_ARG, ": the I_0^4 table's k range");
  if (A.st.host) {
    rc = pairs_positive(ctx, A.who, theta, n_pairs);
    if (rc) return rc;
  }
  HIPCHK(hipSetDevice(ctx->device));
  const NgPlan plan = ng_plan(ctx->cfg, L);
  const NgLayout& G = plan.G;
  const NgTriLayout T = make_ng_tri_layout((int)n_tri);
  const int NK = plan.NK;
  const NgBlocksSizes sizes = ng_blocks_sizes(n_corr, n_pairs, G.N, NK, T.N);
  const size_t sh_kb = (size_t)ng_kb_lds_doubles(G.N, T.N) * sizeof(double);
  if (!fits_lds(&k_ng_blocks_table<false>, plan.sh_table[0]) ||
      (A.n_cross && !fits_lds(&k_ng_blocks_table<true>, plan.sh_table[1])))
    return A.refuse(CHOMP_ERR_ARG, ": cosmo/window_npoints too large for the windows of a block");
  if (!fits_lds(&k_ng_blocks_kb, sh_kb))
    return A.refuse(CHOMP_ERR_ARG, ": kernel_npoints too large for the rows of the two tables");
  NgBlocksState& B = ctx->ng_blocks;
  rc = A.begin(B, sizes.slabs, sizes.kb, epoch);
  if (!rc) rc = ensure(ctx, B.d_tri, sizes.tri);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(B.d_tri + T.tab, tri_table, n_tri * n_tri * sizeof(double),
                        hipMemcpyHostToDevice, ctx->stream));
  rc = A.place(theta, out);
  if (rc) return rc;
  B.G = G;
  unsigned* d_status = epoch ? (unsigned*)ctx->d_status : nullptr;
  hipLaunchKernelGGL(k_ng_tri, dim3(1), dim3(256), 0, ctx->stream, T, tri_k_min, tri_k_max, B.d_tri);
  A.lists(&k_ng_blocks_prep<false>, &k_ng_blocks_prep<true>, 0, {0, 0}, G, ln_ktheta_min,
          ln_ktheta_max, j0_limit, B.d, d_status);
  A.lists(&k_ng_blocks_table<false>, &k_ng_blocks_table<true>, plan.n_tab, plan.sh_table, G,
          ctx->d_j0, B.d, d_status);
  hipLaunchKernelGGL(k_ng_blocks_bicubic, dim3(A.Z), dim3(256), 0, ctx->stream, G, B.d);
  hipLaunchKernelGGL(k_ng_blocks_kb, dim3((unsigned)NK, (unsigned)n_pairs, A.Z), dim3(256), sh_kb,
                     ctx->stream, ctx->cfg, G, T, A.nc, A.d_index, B.d, B.d_tri, tri_k_min,
                     tri_k_max, A.d_theta, A.d_theta + n_pairs, A.d_knots, A.d_lev, d_status);
  return A.finish(B, plan.sh_outer, area);
}

// One block of the last chomp_covariance_ng_blocks (host arrays, any may be NULL).
int chomp_covariance_ng_blocks_table(chomp_ctx* ctx, size_t block, double* info, double* table,
                                     double* levels, double* table_min, double* kb_knots,
                                     double* kb_levels) {
  if (!ctx) return CHOMP_ERR_ARG;
  const NgBlocksState& B = ctx->ng_blocks;
  return term_blocks_table(ctx, "covariance_ng_blocks", B, B.G, block, info, table, levels, table_min,
                           kNgMin, kb_knots, kb_levels);
}
