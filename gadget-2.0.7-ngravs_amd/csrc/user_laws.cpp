// user_laws.cpp -- host side of the user-defined force laws (ngravs_create_with_laws).
//
// The reference calls its laws through `gravity` pointers (allvars.h:134-146); a model's own ngravs.c wires its own functions
// there.  The device cannot call host code, so each user law is sampled here into piecewise polynomials (engine.hpp UserTabs)
// which the kernels evaluate: the r-space force as g(r) = r^2 accel(1, 1, r^2, r, 1) over octaves of r, the softened force per
// distinct softening length over u = r/h in [0, 1).  Degree 7 at the Chebyshev nodes of every sub-interval; the number of
// sub-intervals is doubled until the fit agrees with the callback to UL_TOL at check points between the nodes.
#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>
#include "engine.hpp"

#define UL_TOL 1e-11        // relative deviation allowed at the check points (the tests ask for 1e-9 at random r)
#define UL_S_MIN 32
#define UL_S_MAX 2048
#define UL_FAIL 1e-9        // ... and the deviation at which a law is refused rather than evaluated from its tables

// degree-7 interpolant of phi at the Chebyshev nodes of [-1, 1], as monomial coefficients c[0..7]
template <typename F> static void cheb_fit(F &&phi, double *c)
{
  double v[UL_NC], a[UL_NC];
  for(int j = 0; j < UL_NC; j++)
    v[j] = phi(cos(M_PI * (j + 0.5) / UL_NC));
  for(int k = 0; k < UL_NC; k++)
    {
      double s = 0;
      for(int j = 0; j < UL_NC; j++)
        s += v[j] * cos(M_PI * k * (j + 0.5) / UL_NC);
      a[k] = s * (k == 0 ? 1.0 : 2.0) / UL_NC;
    }
  // T_k as monomials: T_0 = 1, T_1 = t, T_k = 2 t T_{k-1} - T_{k-2}
  double T[UL_NC][UL_NC] = {};
  T[0][0] = 1;
  T[1][1] = 1;
  for(int k = 2; k < UL_NC; k++)
    for(int j = 0; j < UL_NC; j++)
      T[k][j] = (j > 0 ? 2 * T[k - 1][j - 1] : 0.0) - T[k - 2][j];
  for(int j = 0; j < UL_NC; j++)
    {
      c[j] = 0;
      for(int k = 0; k < UL_NC; k++)
        c[j] += a[k] * T[k][j];
    }
}

// fit phi(x) on n equal sub-intervals of a range (x(j, t): the point of sub-interval j at t in [-1, 1]) into out; returns the
// largest relative deviation at the check points, relative to the sub-interval's largest |value|
template <typename X, typename F> static double fit_run(int n, X &&x, F &&phi, double *out)
{
  static const double chk[3] = {0.913, -0.547, 0.171};
  double worst = 0;
  for(int j = 0; j < n; j++)
    {
      double *c = out + (size_t)j * UL_NC, scale = 0;
      cheb_fit([&](double t) {
        const double v = phi(x(j, t));
        scale = fmax(scale, fabs(v));
        return v;
      }, c);
      for(double t : chk)
        {
          const double v = phi(x(j, t)), d = fabs(ul_poly(c, t) - v);
          const double s = fmax(scale, fabs(v));
          if(s > 0)
            worst = fmax(worst, d / s);
          else if(d > 0 || v != v)
            worst = INFINITY;
        }
    }
  return worst;
}

// r-space table of one law over octaves e_lo .. e_lo + n_oct - 1 with S sub-intervals each
// (pot: a PotentialFxns function instead, as p(r) = r pot(1, 1, 0, r, 1))
static double fit_accel(ngravs_gravity_fn f, bool pot, int e_lo, int n_oct, int S, double *out)
{
  double worst = 0;
  for(int o = 0; o < n_oct; o++)
    {
      const int e = e_lo + o;
      auto x = [&](int j, double t) { return ldexp(0.5 + (j + 0.5 * (t + 1)) / (2.0 * S), e); };
      auto g = [&](double r) { return pot ? r * f(1.0, 1.0, 0.0, r, 1) : r * r * f(1.0, 1.0, r * r, r, 1); };
      worst = fmax(worst, fit_run(S, x, g, out + (size_t)o * S * UL_NC));
    }
  return worst;
}
static double fit_spline(ngravs_gravity_fn f, double h, int S, double *out)
{
  auto x = [&](int j, double t) { return (j + 0.5 * (t + 1)) / S; };
  auto s = [&](double u) { return f(1.0, 1.0, h, u * h, 1); };
  return fit_run(S, x, s, out);
}

// octave layout covering [r_lo, r_hi]: r in octave e when 2^(e-1) <= r < 2^e
static void octaves(double r_lo, double r_hi, int *e_lo, int *n_oct)
{
  int a, b;
  (void)frexp(r_lo, &a);
  (void)frexp(r_hi, &b);
  *e_lo = a;
  *n_oct = b - a + 1;
}

// distinct positive softening lengths (at most NGRAVS_NTYPES)
static int distinct_soft(const double *fs, double *h)
{
  int nh = 0;
  for(int t = 0; t < NGRAVS_NTYPES; t++)
    {
      bool seen = !(fs[t] > 0);
      for(int q = 0; q < nh && !seen; q++)
        seen = h[q] == fs[t];
      if(!seen)
        h[nh++] = fs[t];
    }
  return nh;
}

// Build the accel tables of every ACCEL (POT) entry and the spline tables of every SPLINE (POT_SPLINE) entry of a registry into host memory.
// r_hi: largest r the walks can evaluate.  Returns the largest check-point deviation.
static double build_tables(const ngravs_user_fn_t *fns, int nfns, const double *fsoft, double r_hi, UserTabs *ut, std::vector<double> &h)
{
  double hs[NGRAVS_NTYPES];
  const int nh = distinct_soft(fsoft, hs);
  double r_lo = INFINITY;
  for(int q = 0; q < nh; q++)
    r_lo = fmin(r_lo, hs[q]);
  if(!(r_lo < INFINITY))
    r_lo = ldexp(r_hi, -30);   // no softening: the table starts 30 octaves below its end (smaller r clamp to the first octave)
  r_lo = fmin(r_lo, 0.5 * r_hi);
  int e_lo, n_oct;
  octaves(r_lo, r_hi, &e_lo, &n_oct);
  double worst = 0;
  int S = UL_S_MIN, Ss = UL_S_MIN;
  std::vector<double> acc, spl;
  for(;;)
    {
      acc.assign((size_t)nfns * n_oct * S * UL_NC, 0.0);
      double w = 0;
      for(int k = 0; k < nfns; k++)
        if(fns[k].kind == NGRAVS_USER_ACCEL || fns[k].kind == NGRAVS_USER_POT)
          w = fmax(w, fit_accel(fns[k].fn, fns[k].kind == NGRAVS_USER_POT, e_lo, n_oct, S, acc.data() + (size_t)k * n_oct * S * UL_NC));
      if(w <= UL_TOL || S >= UL_S_MAX)
        {
          worst = fmax(worst, w);
          break;
        }
      S *= 2;
    }
  for(;;)
    {
      spl.assign((size_t)nfns * nh * Ss * UL_NC, 0.0);
      double w = 0;
      for(int k = 0; k < nfns; k++)
        if(fns[k].kind == NGRAVS_USER_SPLINE || fns[k].kind == NGRAVS_USER_POT_SPLINE)
          for(int q = 0; q < nh; q++)
            w = fmax(w, fit_spline(fns[k].fn, hs[q], Ss, spl.data() + ((size_t)k * nh + q) * Ss * UL_NC));
      if(w <= UL_TOL || Ss >= UL_S_MAX)
        {
          worst = fmax(worst, w);
          break;
        }
      Ss *= 2;
    }
  h.assign(acc.begin(), acc.end());
  h.insert(h.end(), spl.begin(), spl.end());
  *ut = UserTabs{};
  ut->e_lo = e_lo;
  ut->n_oct = n_oct;
  ut->S = S;
  ut->nh = nh;
  ut->Ss = Ss;
  for(int q = 0; q < nh; q++)
    ut->h[q] = hs[q];
  ut->coef = nullptr;
  ut->spl = (const double *)(uintptr_t)(acc.size() * sizeof(double));   // offset; rebased by the caller
  return worst;
}

int user_green_ensure(ngravs_ctx *c)
{
  const ngravs_config_t &cfg = c->cfg;
  bool any = false;
  for(int a = 0; a < cfg.n_gravs; a++)
    for(int b = 0; b < cfg.n_gravs; b++)
      any = any || cfg.law_greens[a][b] >= NGRAVS_LAW_USER0;
  if(!any || !cfg.pmgrid || c->user_green_nk2 > 0)
    return NGRAVS_OK;
  // pm_periodic.c:440-490: k2 = kx^2 + ky^2 + kz^2 with |k.| <= N/2 is an integer; GreensFxns(MassTable[a], MassTable[b], k2,
  // sqrt(k2), 1) -- independent of the masses (checked at creation)
  const long long half = cfg.pmgrid / 2, nk2 = 3 * half * half + 1;
  const int nfns = (int)c->user_fns.size();
  std::vector<double> h((size_t)nfns * nk2, 0.0);
  for(int k = 0; k < nfns; k++)
    if(c->user_fns[k].kind == NGRAVS_USER_GREENS)
      for(long long q = 1; q < nk2; q++)
        h[(size_t)k * nk2 + q] = c->user_fns[k].fn(1.0, 1.0, (double)q, sqrt((double)q), 1);
  if(c->user_green.ensure(h.size()))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipMemcpyAsync(c->user_green.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->user_green_nk2 = nk2;
  return NGRAVS_OK;
}

// the device tables of one registry (the force laws', the potential companions'): (re)built when r_need or the softenings are
// not covered by what is there
static int registry_tables_ensure(ngravs_ctx *c, const std::vector<ngravs_user_fn_t> &fns, double r_need, const char *what,
                                  DevBuf<double> &tab, UserTabs &cur, bool &ready, double *soft)
{
  bool same_soft = true;
  for(int t = 0; t < NGRAVS_NTYPES; t++)
    same_soft = same_soft && soft[t] == c->cfg.force_softening[t];
  const double top = ready ? ldexp(1.0, cur.e_lo + cur.n_oct - 1) : 0.0;
  if(ready && same_soft && r_need < top)
    return NGRAVS_OK;
  // grow geometrically so that a slowly expanding domain re-tabulates rarely
  const double r_hi = fmax(r_need, 2.0 * top);
  std::vector<double> h;
  UserTabs ut;
  const double worst = build_tables(fns.data(), (int)fns.size(), c->cfg.force_softening, r_hi > 0 ? r_hi : 1.0, &ut, h);
  if(!(worst <= UL_FAIL))
    {
      ngravs_report(c, NGRAVS_ERR_WIRING, std::string(what) + " cannot be tabulated to 1e-9 with " + std::to_string(UL_S_MAX) +
                                               " sub-intervals per octave / softening (a kink or a steep feature?): deviation " +
                                               std::to_string(worst));
      return NGRAVS_ERR_WIRING;
    }
  const size_t spl_off = (size_t)(uintptr_t)ut.spl / sizeof(double);
  if(tab.ensure(h.size() + 1))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipMemcpyAsync(tab.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  ut.coef = tab.p;
  ut.spl = tab.p + spl_off;
  cur = ut;
  for(int t = 0; t < NGRAVS_NTYPES; t++)
    soft[t] = c->cfg.force_softening[t];
  ready = true;
  return NGRAVS_OK;
}

double table_reach(const ngravs_ctx *c, bool shortrange, double far)
{
  if(shortrange && c->cfg.pmgrid)
    return 1.25 * 6.0 * c->asmth;   // TreePM: r < NTAB / asmthfac = 6 Asmth (forcetree.c:1962-1967)
  if(c->cfg.periodic)
    return 1.25 * 0.5 * sqrt(3.0) * c->cfg.box_size;   // the nearest image is at most half a box diagonal away
  // the diagonal of the domain cube (drifted particles of a refit tree may leave it a little; beyond the table's end the last
  // octave's polynomial is used), or the farthest target, which may lie outside the cube, against the cube's far corner.
  // (A mesh implies periodic boundaries, capi.hip refuses anything else: a direct sum never comes here with a mesh.  The
  // association is the force walks'; the potential walk used to write 1.25 * (sqrt(3.0) * dom[6]), at most an ulp away.)
  return fmax(1.25 * sqrt(3.0) * c->dom[6], 1.25 * (far + 0.5 * sqrt(3.0) * c->dom[6]));
}

int user_tables_ensure(ngravs_ctx *c, double r_need)
{
  if(c->user_fns.empty() || !cfg_has_user(c->cfg))
    return NGRAVS_OK;
  return registry_tables_ensure(c, c->user_fns, r_need, "a user-defined law", c->user_tab, c->user_ut, c->user_ready, c->user_soft);
}

int user_pot_tables_ensure(ngravs_ctx *c, double r_need)
{
  if(c->upot_fns.empty())
    return NGRAVS_OK;
  return registry_tables_ensure(c, c->upot_fns, r_need, "a potential function of the model (ngravs_create_with_potentials)", c->upot_tab,
                                c->upot_ut, c->upot_ready, c->upot_soft);
}

extern "C" int ngravs_user_table_eval(const ngravs_user_fn_t *fn, double r_lo, double r_hi, double h, const double *r, int64_t n,
                                      double *out, double *max_err)
{
  if(!fn || !fn->fn || !r || !out || n < 0)
    return NGRAVS_ERR_ARG;
  const bool over_r = fn->kind == NGRAVS_USER_ACCEL || fn->kind == NGRAVS_USER_POT;
  if(!over_r && fn->kind != NGRAVS_USER_SPLINE && fn->kind != NGRAVS_USER_POT_SPLINE)
    return NGRAVS_ERR_ARG;
  double fs[NGRAVS_NTYPES] = {0, 0, 0, 0, 0, 0};
  if(over_r)
    {
      if(!(r_lo > 0) || !(r_hi > r_lo))
        return NGRAVS_ERR_ARG;
      fs[0] = r_lo;
    }
  else
    {
      if(!(h > 0))
        return NGRAVS_ERR_ARG;
      fs[0] = h;
    }
  std::vector<double> tab;
  UserTabs ut;
  const double w = build_tables(fn, 1, fs, over_r ? r_hi : 2 * h, &ut, tab);
  const size_t spl_off = (size_t)(uintptr_t)ut.spl / sizeof(double);
  ut.coef = tab.data();
  ut.spl = tab.data() + spl_off;
  for(int64_t i = 0; i < n; i++)
    out[i] = fn->kind == NGRAVS_USER_ACCEL ? ul_g(ut, 0, r[i]) / (r[i] * r[i])
                                           : (fn->kind == NGRAVS_USER_POT ? ul_g(ut, 0, r[i]) / r[i] : ul_spline(ut, 0, h, r[i]));
  if(max_err)
    *max_err = w;
  return NGRAVS_OK;
}

// ---- the model's lattice corrections (ngravs_create_with_lattice) ------------------------------------------------------------
// lattice_init (forcetree.c:3611-3793): LatticeForce[l][m](i, j, k, x, force) at x = 0.5 (i, j, k) / NGRAVS_EN, divided by
// BoxSize^2; the layout of k_lattice_table, [3][65^3] with point (i, j, k) at (i * 65 + j) * 65 + k
#define ULAT_EN 64
#define ULAT_E1 (ULAT_EN + 1)
#define ULAT_THREADS 16   // the most host threads a tabulation uses (a job's share of the machine, not the machine)

int user_lattice_tabulate(ngravs_lattice_fn fn, double box, double *out, std::string &why)
{
  const long long npts = (long long)ULAT_E1 * ULAT_E1 * ULAT_E1;
  const double L2 = box * box;
  const unsigned hc = std::thread::hardware_concurrency();
  const int nth = (int)std::max(1u, std::min((unsigned)ULAT_THREADS, hc));
  std::vector<long long> bad(nth, -1);   // per thread: the first point whose sample is not finite
  auto work = [&](int t) {
    for(long long n = npts * t / nth; n < npts * (t + 1) / nth; n++)
      {
        const int i = (int)(n / (ULAT_E1 * ULAT_E1)), j = (int)((n / ULAT_E1) % ULAT_E1), k = (int)(n % ULAT_E1);
        double x[3] = {0.5 * ((double)i) / ULAT_EN, 0.5 * ((double)j) / ULAT_EN, 0.5 * ((double)k) / ULAT_EN};
        double f[3] = {0, 0, 0};   // the reference's yukawa_lattice_force returns at the origin without writing it
        fn(i, j, k, x, f);
        if(!std::isfinite(f[0]) || !std::isfinite(f[1]) || !std::isfinite(f[2]))
          {
            bad[t] = n;
            return;
          }
        for(int c = 0; c < 3; c++)
          out[c * npts + n] = f[c] / L2;
      }
  };
  std::vector<std::thread> th;
  for(int t = 1; t < nth; t++)
    {
      try
        {
          th.emplace_back(work, t);
        }
      catch(...)
        {
          work(t);   // no thread to be had: this one does the share
        }
    }
  work(0);
  for(auto &x : th)
    x.join();
  for(int t = 0; t < nth; t++)
    if(bad[t] >= 0)
      {
        const long long n = bad[t];
        why = "lattice function: non-finite force at point (" + std::to_string(n / (ULAT_E1 * ULAT_E1)) + ", " +
              std::to_string((n / ULAT_E1) % ULAT_E1) + ", " + std::to_string(n % ULAT_E1) + ")";
        return NGRAVS_ERR_WIRING;
      }
  return NGRAVS_OK;
}

extern "C" int ngravs_user_lattice_table(ngravs_lattice_fn fn, double box_size, double *out)
{
  if(!fn || !out || !(box_size > 0))
    return NGRAVS_ERR_ARG;
  std::string why;
  const int rc = user_lattice_tabulate(fn, box_size, out, why);
  if(rc)
    ngravs_report(nullptr, rc, why);
  return rc;
}

ngravs_lattice_fn user_lattice_fn(const ngravs_ctx *c, int a, int b)
{
  for(const ngravs_user_lattice_t &e : c->user_lat)
    if(e.target == a && e.source == b)
      return e.fn;
  return nullptr;
}

bool user_lattice_complete(const ngravs_ctx *c)
{
  const int ng = c->cfg.n_gravs;
  for(int a = 0; a < ng; a++)
    for(int b = 0; b < ng; b++)
      if(c->cfg.law_accel[a][b] >= NGRAVS_LAW_USER0 && !user_lattice_fn(c, a, b))
        return false;
  return true;
}

// ---- the model's potential companions (ngravs_create_with_potentials) -------------------------------------------------------
// lattice_init's potcorr (forcetree.c:3699-3702): LatticePotential[l][m](x) at x = 0.5 (i, j, k) / NGRAVS_EN, the origin
// LatticeZero[l][m], both divided by BoxSize; the layout of k_lattice_pot_table
int user_pot_lattice_tabulate(ngravs_lattice_pot_fn fn, double zero, double box, double *out, std::string &why)
{
  const long long npts = (long long)ULAT_E1 * ULAT_E1 * ULAT_E1;
  const unsigned hc = std::thread::hardware_concurrency();
  const int nth = (int)std::max(1u, std::min((unsigned)ULAT_THREADS, hc));
  std::vector<long long> bad(nth, -1);   // per thread: the first point whose sample is not finite
  auto work = [&](int t) {
    for(long long n = npts * t / nth; n < npts * (t + 1) / nth; n++)
      {
        const int i = (int)(n / (ULAT_E1 * ULAT_E1)), j = (int)((n / ULAT_E1) % ULAT_E1), k = (int)(n % ULAT_E1);
        double x[3] = {0.5 * ((double)i) / ULAT_EN, 0.5 * ((double)j) / ULAT_EN, 0.5 * ((double)k) / ULAT_EN};
        const double v = n == 0 ? zero : fn(x);   // the origin never calls the function
        if(!std::isfinite(v))
          {
            bad[t] = n;
            return;
          }
        out[n] = v / box;
      }
  };
  std::vector<std::thread> th;
  for(int t = 1; t < nth; t++)
    {
      try
        {
          th.emplace_back(work, t);
        }
      catch(...)
        {
          work(t);   // no thread to be had: this one does the share
        }
    }
  work(0);
  for(auto &x : th)
    x.join();
  for(int t = 0; t < nth; t++)
    if(bad[t] >= 0)
      {
        const long long n = bad[t];
        why = "lattice potential: non-finite value at point (" + std::to_string(n / (ULAT_E1 * ULAT_E1)) + ", " +
              std::to_string((n / ULAT_E1) % ULAT_E1) + ", " + std::to_string(n % ULAT_E1) + ")";
        return NGRAVS_ERR_WIRING;
      }
  return NGRAVS_OK;
}

const ngravs_user_potential_t *user_pot_entry(const ngravs_ctx *c, int a, int b)
{
  for(const ngravs_user_potential_t &e : c->user_pot)
    if(e.target == a && e.source == b)
      return &e;
  return nullptr;
}

// the distinct pot and pot_spline functions of the entries, each tabulated once
void user_pot_registry(ngravs_ctx *c)
{
  c->upot_fns.clear();
  auto add = [&](int kind, ngravs_gravity_fn f) {
    for(const ngravs_user_fn_t &u : c->upot_fns)
      if(u.kind == kind && u.fn == f)
        return;
    c->upot_fns.push_back(ngravs_user_fn_t{kind, 0, f});
  };
  for(const ngravs_user_potential_t &e : c->user_pot)
    {
      add(NGRAVS_USER_POT, e.pot);
      add(NGRAVS_USER_POT_SPLINE, e.pot_spline);
    }
}

void user_pot_maps(const ngravs_ctx *c, PotUser *pu)
{
  auto find = [&](int kind, ngravs_gravity_fn f) {
    for(size_t k = 0; k < c->upot_fns.size(); k++)
      if(c->upot_fns[k].kind == kind && c->upot_fns[k].fn == f)
        return (int)k;
    return -1;
  };
  for(int a = 0; a < NG_MAX; a++)
    for(int b = 0; b < NG_MAX; b++)
      {
        const ngravs_user_potential_t *e = a < c->cfg.n_gravs && b < c->cfg.n_gravs ? user_pot_entry(c, a, b) : nullptr;
        pu->kp[a][b] = e ? find(NGRAVS_USER_POT, e->pot) : -1;
        pu->ks[a][b] = e ? find(NGRAVS_USER_POT_SPLINE, e->pot_spline) : -1;
      }
  pu->ut = c->upot_ut;
}

static bool close_to(double a, double b);

int user_check_potentials(const ngravs_config_t *cfg, const ngravs_user_potential_t *pots, int npot, std::string &why)
{
  if(npot < 0 || (npot > 0 && !pots))
    {
      why = "potential entries: a negative count or no array";
      return NGRAVS_ERR_ARG;
    }
  const int ng = cfg->n_gravs;
  auto name = [&](int e) {
    return "potential entry " + std::to_string(e) + " [" + std::to_string(pots[e].target) + "][" + std::to_string(pots[e].source) + "]";
  };
  for(int e = 0; e < npot; e++)
    {
      const int a = pots[e].target, b = pots[e].source;
      if(a < 0 || a >= ng || b < 0 || b >= ng)
        {
          why = name(e) + ": species pair out of range";
          return NGRAVS_ERR_WIRING;
        }
      for(int q = 0; q < e; q++)
        if(pots[q].target == a && pots[q].source == b)
          {
            why = name(e) + ": a second entry for this pair (entry " + std::to_string(q) + ")";
            return NGRAVS_ERR_WIRING;
          }
      if(cfg->law_accel[a][b] == NGRAVS_LAW_NONE)
        {
          why = name(e) + ": law_accel of the pair is NONE (nothing is wired there)";
          return NGRAVS_ERR_WIRING;
        }
      if(!pots[e].pot || !pots[e].pot_spline)
        {
          why = name(e) + ": no pot or no pot_spline function";
          return NGRAVS_ERR_WIRING;
        }
      if(pots[e].lattice_pot && !cfg->periodic)
        {
          why = name(e) + ": a lattice potential in a non-periodic configuration";
          return NGRAVS_ERR_WIRING;
        }
      if(!pots[e].lattice_pot && cfg->periodic && !cfg->pmgrid)
        {
          why = name(e) + ": a periodic tree-only run needs the pair's lattice_pot (the reference's LatticePotential)";
          return NGRAVS_ERR_WIRING;
        }
      if(!std::isfinite(pots[e].lattice_zero))
        {
          why = name(e) + ": lattice_zero is not finite";
          return NGRAVS_ERR_WIRING;
        }
      bool mirrored = a == b || cfg->law_accel[b][a] == NGRAVS_LAW_NONE;
      for(int q = 0; q < npot && !mirrored; q++)
        mirrored = pots[q].target == b && pots[q].source == a;
      if(!mirrored)
        {
          why = name(e) + ": the mirrored pair has no entry (the two are probed against each other, ngravs_core.c:389-413)";
          return NGRAVS_ERR_WIRING;
        }
    }
  // ngravs_core.c:389, :408-413 for the pairs that have entries on both sides
  for(int e = 0; e < npot; e++)
    for(int q = 0; q < e; q++)
      if(pots[q].target == pots[e].source && pots[q].source == pots[e].target)
        {
          if(!(pots[e].pot(1, 1, 0.5, 3, 1) == pots[q].pot(1, 1, 0.5, 3, 1)) ||
             !(pots[e].pot_spline(1, 1, 0.5, 3, 1) == pots[q].pot_spline(1, 1, 0.5, 3, 1)))
            {
              why = name(e) + ": potential table violates Newton's third law against entry " + std::to_string(q) + " (ngravs_core.c:408-413)";
              return NGRAVS_ERR_WIRING;
            }
          if(pots[e].lattice_pot != pots[q].lattice_pot || !(pots[e].lattice_zero == pots[q].lattice_zero))
            {
              why = name(e) + ": lattice_pot or lattice_zero differs from entry " + std::to_string(q) + " of the mirrored pair (ngravs_core.c:389)";
              return NGRAVS_ERR_WIRING;
            }
        }
  // what a tree can represent: linear in the source mass, independent of the target mass and of N (the probes of the force laws)
  for(int e = 0; e < npot; e++)
    {
      auto probe = [&](ngravs_gravity_fn f, double x, double r) -> bool {
        const double v = f(1, 1, x, r, 1);
        return std::isfinite(v) && close_to(f(1, 2, x, r, 1), 2 * v) && close_to(f(1, 0.25, x, r, 1), 0.25 * v) &&
               close_to(f(3, 1, x, r, 1), v) && close_to(f(1, 1, x, r, 7), v);
      };
      bool ok = true, no_h = true;
      for(double r : {1e-3, 0.05, 0.7, 3.0, 40.0, 900.0})
        {
          ok = ok && probe(pots[e].pot, 0.5 * r, r);
          no_h = no_h && close_to(pots[e].pot(1, 1, 0.5 * r, r, 1), pots[e].pot(1, 1, 0.0, r, 1));
        }
      for(double u : {0.0, 0.05, 0.3, 0.6, 0.95})
        ok = ok && probe(pots[e].pot_spline, 1.0, u);
      if(!ok)
        {
          why = name(e) + ": the tree needs a potential linear in the source mass and independent of the target mass and of N "
                          "(a node's monopole is a mass sum)";
          return NGRAVS_ERR_WIRING;
        }
      if(!no_h)
        {
          why = name(e) + ": pot depends on its softening argument h (it is tabulated over r alone, for r >= h)";
          return NGRAVS_ERR_WIRING;
        }
    }
  return NGRAVS_OK;
}

// ---- the checks of ngravs_create_with_laws ----------------------------------------------------------------------------------
static bool is_user(int id) { return id >= NGRAVS_LAW_USER0; }

// built-in laws at the probe of ngravs_core.c:367-403 (the reference's own functions, ngravs.c:351-455, 826-885)
static bool builtin_value(const ngravs_config_t *cfg, int kind, int id, double t, double s, double x, double r, double *v)
{
  const double ym = cfg->box_size > 0 ? cfg->yukawa_imass / cfg->box_size : 0.0;
  if(id == 0)
    {
      *v = 0;
      return true;
    }
  if(kind == NGRAVS_USER_ACCEL)
    switch(id)
      {
      case NGRAVS_LAW_NEWTON: *v = s / x; return true;
      case NGRAVS_LAW_NEG_NEWTON: *v = -s / x; return true;
      case NGRAVS_LAW_YUKAWA: *v = s * exp(-r * ym) * (ym / r + 1.0 / x); return true;
      case NGRAVS_LAW_COLOYUK: *v = s * exp(-r * ym) * (ym / r + 1.0 / x) + s / x; return true;
      default: return false;
      }
  if(kind == NGRAVS_USER_SPLINE && (id == NGRAVS_SPLINE_PLUMMER || id == NGRAVS_SPLINE_NEG_PLUMMER))
    {
      const double hi = 1 / x;
      double u = r * hi, w;
      if(u < 0.5)
        w = s * hi * hi * hi * (10.666666666667 + u * u * (32.0 * u - 38.4));
      else
        w = s * hi * hi * hi * (21.333333333333 - 48.0 * u + 38.4 * u * u - 10.666666666667 * u * u * u - 0.066666666667 / (u * u * u));
      *v = id == NGRAVS_SPLINE_NEG_PLUMMER ? -w : w;
      return true;
    }
  if(kind == NGRAVS_USER_GREENS && (id == NGRAVS_LAW_NEWTON || id == NGRAVS_LAW_NEG_NEWTON))
    {
      *v = id == NGRAVS_LAW_NEWTON ? 1.0 / x : -1.0 / x;   // pgdelta / neg_pgdelta
      return true;
    }
  if(kind == NGRAVS_USER_NORMED && (id == NGRAVS_LAW_NEWTON || id == NGRAVS_LAW_NEG_NEWTON))
    {
      *v = id == NGRAVS_LAW_NEWTON ? 1.0 : -1.0;             // normed_pgdelta / its negative
      return true;
    }
  return false;
}

static bool close_to(double a, double b) { return a == b || fabs(a - b) <= 1e-12 * fmax(fabs(a), fabs(b)); }

// the lattice entries of ngravs_create_with_lattice
static int user_check_lattice(const ngravs_config_t *cfg, const ngravs_user_lattice_t *lat, int nlat, std::string &why)
{
  if(nlat < 0 || (nlat > 0 && !lat))
    {
      why = "lattice entries: a negative count or no array";
      return NGRAVS_ERR_ARG;
    }
  const int ng = cfg->n_gravs;
  for(int e = 0; e < nlat; e++)
    {
      const int a = lat[e].target, b = lat[e].source;
      const std::string name = "lattice entry " + std::to_string(e) + " [" + std::to_string(a) + "][" + std::to_string(b) + "]";
      if(a < 0 || a >= ng || b < 0 || b >= ng || !lat[e].fn)
        {
          why = name + ": species pair out of range or no function";
          return NGRAVS_ERR_WIRING;
        }
      if(!cfg->periodic)
        {
          why = name + ": lattice corrections in a non-periodic configuration";
          return NGRAVS_ERR_WIRING;
        }
      for(int q = 0; q < e; q++)
        if(lat[q].target == a && lat[q].source == b)
          {
            why = name + ": a second entry for this pair (entry " + std::to_string(q) + ")";
            return NGRAVS_ERR_WIRING;
          }
      if(!is_user(cfg->law_accel[a][b]))
        {
          why = name + ": law_accel of the pair is the built-in id " + std::to_string(cfg->law_accel[a][b]) +
                " (its lattice correction is the library's own)";
          return NGRAVS_ERR_WIRING;
        }
    }
  return NGRAVS_OK;
}

int user_check_config(const ngravs_config_t *cfg, const ngravs_user_fn_t *fns, int nfns, const ngravs_user_lattice_t *lat, int nlat,
                      std::string &why)
{
  if(nfns < 0 || nfns > NGRAVS_MAX_USER_FNS || (nfns > 0 && !fns))
    {
      why = "user-law registry: at most NGRAVS_MAX_USER_FNS entries";
      return NGRAVS_ERR_ARG;
    }
  if(int rc = user_check_lattice(cfg, lat, nlat, why))
    return rc;
  for(int k = 0; k < nfns; k++)
    if(!fns[k].fn || fns[k].kind < NGRAVS_USER_ACCEL || fns[k].kind > NGRAVS_USER_NORMED)
      {
        why = "user-law registry entry " + std::to_string(k) + ": no function or unknown kind";
        return NGRAVS_ERR_ARG;
      }
  const int ng = cfg->n_gravs;
  const int(*tabs[4])[NGRAVS_MAX_GRAVS] = {cfg->law_accel, cfg->law_spline, cfg->law_greens, cfg->law_normed};
  static const char *names[4] = {"law_accel", "law_spline", "law_greens", "law_normed"};
  bool any = false;
  for(int kind = 0; kind < 4; kind++)
    for(int i = 0; i < ng; i++)
      for(int j = 0; j < ng; j++)
        {
          const int id = tabs[kind][i][j];
          if(!is_user(id))
            continue;
          any = true;
          const int k = id - NGRAVS_LAW_USER0;
          if(k >= nfns || fns[k].kind != kind)
            {
              why = std::string(names[kind]) + "[" + std::to_string(i) + "][" + std::to_string(j) + "] = " + std::to_string(id) +
                    (k >= nfns ? ": user id outside the registry" : ": registry entry of another kind");
              return NGRAVS_ERR_WIRING;
            }
        }
  if(!any)
    return NGRAVS_OK;
  if(cfg->periodic && !cfg->pmgrid)
    for(int i = 0; i < ng; i++)
      for(int j = 0; j < ng; j++)
        {
          bool has = false;
          for(int e = 0; e < nlat && !has; e++)
            has = lat[e].target == i && lat[e].source == j;
          if(is_user(cfg->law_accel[i][j]) && !has)
            {
              why = "law_accel[" + std::to_string(i) + "][" + std::to_string(j) +
                    "] is a user-defined law in a periodic tree-only run: its lattice correction needs the model's own "
                    "LatticeForce function (ngravs_create_with_lattice)";
              return NGRAVS_ERR_WIRING;
            }
        }
  // Newton's third law, the reference's probe F[i][j](1,1,0.5,3,1) == F[j][i](1,1,0.5,3,1) (ngravs_core.c:367-403)
  for(int kind = 0; kind < 4; kind++)
    for(int i = 0; i < ng; i++)
      for(int j = 0; j < ng; j++)
        {
          const int a = tabs[kind][i][j], b = tabs[kind][j][i];
          if(!is_user(a) && !is_user(b))
            continue;
          double va, vb;
          bool ok = is_user(a) ? (va = fns[a - NGRAVS_LAW_USER0].fn(1, 1, 0.5, 3, 1), true) : builtin_value(cfg, kind, a, 1, 1, 0.5, 3, &va);
          ok = ok && (is_user(b) ? (vb = fns[b - NGRAVS_LAW_USER0].fn(1, 1, 0.5, 3, 1), true) : builtin_value(cfg, kind, b, 1, 1, 0.5, 3, &vb));
          if(!ok)
            {
              why = std::string(names[kind]) + ": a user law paired with a built-in law that cannot be probed on the host";
              return NGRAVS_ERR_WIRING;
            }
          if(!(va == vb))
            {
              why = std::string(names[kind]) + "[" + std::to_string(i) + "][" + std::to_string(j) +
                    "]: force-law table violates Newton's third law (ngravs_core.c:371-403)";
              return NGRAVS_ERR_WIRING;
            }
        }
  // what a tree can represent: linear in the source mass, independent of the target mass and of N
  for(int k = 0; k < nfns; k++)
    {
      ngravs_gravity_fn f = fns[k].fn;
      auto probe = [&](double x, double r) -> bool {
        const double v = f(1, 1, x, r, 1);
        if(fns[k].kind == NGRAVS_USER_GREENS || fns[k].kind == NGRAVS_USER_NORMED)
          return close_to(f(2, 3, x, r, 1), v) && close_to(f(1, 1, x, r, 7), v);
        return std::isfinite(v) && close_to(f(1, 2, x, r, 1), 2 * v) && close_to(f(1, 0.25, x, r, 1), 0.25 * v) &&
               close_to(f(3, 1, x, r, 1), v) && close_to(f(1, 1, x, r, 7), v);
      };
      bool ok = true;
      if(fns[k].kind == NGRAVS_USER_ACCEL)
        for(double r : {1e-3, 0.05, 0.7, 3.0, 40.0, 900.0})
          ok = ok && probe(r * r, r);
      else if(fns[k].kind == NGRAVS_USER_SPLINE)
        for(double u : {0.05, 0.3, 0.6, 0.95})
          ok = ok && probe(1.0, u);
      else
        for(double k2 : {0.5, 3.0, 40.0})
          ok = ok && probe(k2, sqrt(k2));
      if(!ok)
        {
          why = "user-law registry entry " + std::to_string(k) +
                (fns[k].kind <= NGRAVS_USER_SPLINE
                     ? ": the tree needs a force linear in the source mass and independent of the target mass and of N "
                       "(a node's monopole is a mass sum)"
                     : ": a Green's function must not depend on its mass arguments");
          return NGRAVS_ERR_WIRING;
        }
    }
  return NGRAVS_OK;
}

// NormedGreensFxns of a user id for the short-range table (k^2 in the table's units, shortrange_table.cpp)
double user_normed(const ngravs_user_fn_t *fns, int nfns, int law, double k2)
{
  const int k = law - NGRAVS_LAW_USER0;
  if(k < 0 || k >= nfns || fns[k].kind != NGRAVS_USER_NORMED)
    return 0.0;
  return fns[k].fn(1.0, 1.0, k2, sqrt(k2), 1);
}
