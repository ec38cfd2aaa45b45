// kernels_potential.hip -- gravitational potentials: P[].Potential of compute_potential() (potential.c:22-345).
//
// What the reference's routines MEAN, not what they do (DESIGN.md §8 lists why they cannot be a parity target):
//   force_treeevaluate_potential            forcetree.c:2560-2768   potential_walk_lane<NG, 0, LATT>
//   force_treeevaluate_potential_shortrange forcetree.c:2871-3150   potential_walk_lane<NG, 1, 0>
//   lattice_pot_corr / ewald_psi            forcetree.c:3895ff, ngravs.c:761-816   lat_pot_lookup / k_lattice_pot_table
//   the tail of compute_potential           potential.c:244-337     k_potential_finish
// The mesh part (pmpotential_periodic) is kernels_pm.hip's pm_solve + k_potential_gather.
//
// The walk is the strict walk's traversal (strict_walk.hpp: the driver, the species offsets, the opening criterion, the reach box,
// the pseudo-node flag -- the code the force walk runs) with the potential walk's own interaction and softening rule and its two
// differences: a periodic tree-only run adds the lattice term in the same visit (no second walk), and the short-range walk
// prunes by the eff_dist box alone -- here with the table's reach.  Wired companions: newtonian_pot,
// neg_newtonian_pot, plummer_pot, neg_plummer_pot (ngravs.c:368-489), as the coefficients cN / cS of WalkParams (+1, -1, 0).
// The USR variants also read the model's own companions (ngravs_create_with_potentials) from the tables user_laws.cpp builds.
#include "engine.hpp"
#include "walk_device.hpp"
#include "strict_walk.hpp"
#include "columns.hpp"

#pragma clang fp contract(off)

#define POT_LAT_SZ ((size_t)LAT_E1 * LAT_E1 * LAT_E1)
#define LATTICE_ZERO 2.8372975   // ngravs.c:133

// plummer_pot (ngravs.c:459-472), literal constants
__device__ __forceinline__ double plummer_pot(double m, double h, double r)
{
  const double h_inv = 1 / h;
  r *= h_inv;
  if(r < 0.5)
    return m * h_inv * (-2.8 + r * r * (5.333333333333 + r * r * (6.4 * r - 9.6)));
  return m * h_inv * (-3.2 + 0.066666666667 / r + r * r * (10.666666666667 + r * (-16.0 + r * (9.6 - 2.133333333333 * r))));
}

// ewald_psi (ngravs.c:761-816) at x in box units, summed in its order
__host__ __device__ inline double ewald_psi(const double x[3])
{
  const double alpha = 2.0;
  double sum1 = 0, sum2 = 0;
  for(int n0 = -4; n0 <= 4; n0++)
    for(int n1 = -4; n1 <= 4; n1++)
      for(int n2 = -4; n2 <= 4; n2++)
        {
          const double dx[3] = {x[0] - n0, x[1] - n1, x[2] - n2};
          const double r = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
          sum1 += erfc(alpha * r) / r;
        }
  for(int h0 = -4; h0 <= 4; h0++)
    for(int h1 = -4; h1 <= 4; h1++)
      for(int h2_ = -4; h2_ <= 4; h2_++)
        {
          const double hdotx = x[0] * h0 + x[1] * h1 + x[2] * h2_;
          const int h2 = h0 * h0 + h1 * h1 + h2_ * h2_;
          if(h2 > 0)
            sum2 += 1 / (M_PI * h2) * exp(-M_PI * M_PI * h2 / (alpha * alpha)) * cos(2 * M_PI * hdotx);
        }
  const double r = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  return M_PI / (alpha * alpha) - sum1 - sum2 + 1 / r;
}

// one thread per point of the octant grid: out[E1^3] = sign ewald_psi(x) / BoxSize, the origin LatticeZero (forcetree.c:3699-3702)
__global__ void k_lattice_pot_table(double sign, double box, double *__restrict__ out)
{
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if(n >= LAT_E1 * LAT_E1 * LAT_E1)
    return;
  const int i = n / (LAT_E1 * LAT_E1), j = (n / LAT_E1) % LAT_E1, k = n % LAT_E1;
  const double x[3] = {0.5 * ((double)i) / LAT_EN, 0.5 * ((double)j) / LAT_EN, 0.5 * ((double)k) / LAT_EN};
  out[n] = sign * (n == 0 ? LATTICE_ZERO : ewald_psi(x)) / box;
}

// lattice_pot_corr (forcetree.c:3895-3941): trilinear lookup in the octant table of one species pair, to be multiplied by the mass
__device__ __forceinline__ double lat_pot_lookup(const double *__restrict__ a, double fac_intp, double dx, double dy, double dz)
{
  double u = fabs(dx) * fac_intp, v = fabs(dy) * fac_intp, w = fabs(dz) * fac_intp;
  int i = (int)u, j = (int)v, k = (int)w;
  i = i >= LAT_EN ? LAT_EN - 1 : (i < 0 ? 0 : i);
  j = j >= LAT_EN ? LAT_EN - 1 : (j < 0 ? 0 : j);
  k = k >= LAT_EN ? LAT_EN - 1 : (k < 0 ? 0 : k);
  u -= i;
  v -= j;
  w -= k;
  const double f1 = (1 - u) * (1 - v) * (1 - w), f2 = (1 - u) * (1 - v) * (w), f3 = (1 - u) * (v) * (1 - w), f4 = (1 - u) * (v) * (w),
               f5 = (u) * (1 - v) * (1 - w), f6 = (u) * (1 - v) * (w), f7 = (u) * (v) * (1 - w), f8 = (u) * (v) * (w);
  const size_t o = ((size_t)i * LAT_E1 + j) * LAT_E1 + k, sj = LAT_E1, si = (size_t)LAT_E1 * LAT_E1;
  return a[o] * f1 + a[o + 1] * f2 + a[o + sj] * f3 + a[o + sj + 1] * f4 + a[o + si] * f5 + a[o + si + 1] * f6 + a[o + si + sj] * f7 +
         a[o + si + sj + 1] * f8;
}

// The last kernel argument: the model's potential tables (USR), or a word nobody reads -- the USR = false kernels are the code
// they were before there were such tables
struct NoPotUser
{
  int unused;
};
template <bool USR> using PotUserArg = std::conditional_t<USR, PotUser, NoPotUser>;

// One lane's potential walk for a target given by value: the one body of k_potential_walk (own rows) and k_potential_targets
// (records handed in).  table: PM the long-range potential E [tg][sg][NTAB], LATT the lattice potential [tg][sg][E1^3].
// USR: a pair with an entry of ngravs_create_with_potentials evaluates the entry's two tables (pu), every other pair cN / cS.
template <int NG, bool PM, bool LATT, bool USR>
__device__ __forceinline__ void potential_walk_lane(const TreeView &tv, const double4 *__restrict__ s_pm, const unsigned char *__restrict__ s_type,
                                                    const double *__restrict__ table, const WalkParams &wp, const double utorwpi,
                                                    const double reach, const bool valid, const StrictTarget &T, int *sn, int *ss, int *__restrict__ err_flag,
                                                    const PotUserArg<USR> &pu, double &pot_out, int &nint_out)
{
  const double hT = T.h;
  const int tg = T.tg;
  double pot = 0;
  int nint = 0;
  StrictDfs w;
  w.sn = sn;
  w.ss = ss;

  // USR: the tables of this lane's target species against every source species, one byte each (table + 1; 0: no entry).  The
  // source species of a visit is the same for the whole wave, the target's is the lane's: the piece of the table a lane reads
  // depends on its r anyway, so the coefficients come through vector loads
  unsigned kpk = 0, ksk = 0;
  if constexpr(USR)
    {
#pragma unroll
      for(int g = 0; g < NG; g++)
        {
          kpk |= (unsigned)(pu.kp[tg][g] + 1) << (8 * g);
          ksk |= (unsigned)(pu.ks[tg][g] + 1) << (8 * g);
        }
    }
  // PotentialFxns / PotentialSplines of the pair (tg, g) for a source of mass m
  auto p_far = [&](int g, double m, double r) -> double {
    if constexpr(USR)
      {
        const int k = (int)((kpk >> (8 * g)) & 0xff) - 1;
        if(k >= 0)
          return m * (ul_g(pu.ut, k, r) / r);
      }
    return wp.cN[tg][g] * (m / r);
  };
  auto p_near = [&](int g, double m, double h, double r) -> double {
    if constexpr(USR)
      {
        const int k = (int)((ksk >> (8 * g)) & 0xff) - 1;
        if(k >= 0)
          return m * ul_spline(pu.ut, k, h, r);
      }
    return wp.cS[tg][g] * plummer_pot(m, h, r);
  };

  // one source (particle or one species of a node): forcetree.c:2725-2768 / :3104ff
  auto interact = [&](int g, double dx, double dy, double dz, double r2, double m, double h) -> bool {
    const double r = sqrt(r2);
    if(PM)
      {
        const int tab = (int)(wp.asmthfac * r);
        if(tab >= NTAB || tab < 0)
          return false;
        // the mesh's share of this pair, removed inside h too: the mesh holds it for close pairs and for the particle itself
        const double lr = m * utorwpi * table[((size_t)tg * NG + g) * NTAB + tab];
        if(r >= h)
          pot -= p_far(g, m, r) - lr;
        else
          pot += p_near(g, m, h, r) + lr;
      }
    else
      {
        if(r >= h)
          pot -= p_far(g, m, r);
        else
          pot += p_near(g, m, h, r);
        if(LATT)
          pot += m * lat_pot_lookup(table + ((size_t)tg * NG + g) * POT_LAT_SZ, wp.fac_intp, dx, dy, dz);   // forcetree.c:2737
      }
    return true;
  };

  auto do_particle = [&](int p) {
    const double4 q = s_pm[p];   // uniform address -> scalar load
    const int qt = s_type[p];
    if(w.takes_part())
      {
        double dx, dy, dz;
        const double r2 = offset_from(q, T, wp, wp.periodic, dx, dy, dz);
        double h = hT;
        if(h < wp.fsoft[qt])
          h = wp.fsoft[qt];
        const bool added = interact(wp.t2g[qt], dx, dy, dz, r2, q.w, h);
        if(added || !PM)
          nint++;
      }
  };

  auto visit = [&](int c) -> bool {
    const int fl = tv.flags[c];
    const double4 geo = tv.geo[c];
    double4 mom[NG];
    node_moments<NG>(tv, c, mom);
    bool open = false;
    const bool takes_part = w.takes_part();
    if(takes_part)
      {
        double dx[NG], dy[NG], dz[NG], r2[NG], r2min, r2max, summass;
        species_offsets<NG>(mom, T, wp, wp.periodic, dx, dy, dz, r2, r2min, r2max, summass);
        // pruned: the eff_dist box of forcetree.c:2990-3021 (no test on r2min in front of it), with the reach of the table, 6 Asmth,
        // in the place of rcut = 4.5 Asmth: a cell outside it holds no pair with tab < NTAB, so nothing is lost.  The
        // reference's box drops pairs between the two, each worth erfc(2.25) = 1.5e-3 of its m / r
        bool done = false;
        if(PM)
          {
            if(outside_reach_box(geo, T, wp, reach + 0.5 * geo.w))
              done = true;
          }
        if(!done)
          open = node_opens(geo, T, wp, r2min, summass);
        if(!done && !open)
          {
            double h = hT;
            const int mst = (fl >> 2) & 7;
            if(mst == 7)
              open = true;                                             // empty node: nothing below, harmless
            else
              {
                if(h < wp.fsoft[mst])
                  {
                    h = wp.fsoft[mst];
                    if(r2max < h * h && ((fl >> 5) & 1))               // forcetree.c:2685-2696
                      open = true;
                  }
                if(!open)
                  {
                    bool added = false;
#pragma unroll
                    for(int g = 0; g < NG; g++)
                      if(mom[g].w != 0.0)
                        added |= interact(g, dx[g], dy[g], dz[g], r2[g], mom[g].w, h);
                    if(added || !PM)
                      nint++;
                  }
              }
          }
      }
    const bool wave_open = w.settle(takes_part, open);
    report_pseudo(wave_open, fl, err_flag);   // a top leaf that was not imported (k_walk_strict reports the same)
    return wave_open;
  };
  w.reset(valid);
  w.run(tv, visit, do_particle);
  pot_out = pot;
  nint_out = nint;
}

// targets: ALL own rows [0, n) in Peano order, whatever their active flags, 64 consecutive rows per wave
template <int NG, bool PM, bool LATT, bool USR>
__global__ __launch_bounds__(256) void k_potential_walk(TreeView tv, const double4 *__restrict__ s_pm, const unsigned char *__restrict__ s_type,
                                                        const double *__restrict__ s_oldacc, const double *__restrict__ table, WalkParams wp,
                                                        double utorwpi, double reach, long long n, double *__restrict__ r_pot, int *__restrict__ r_nint,
                                                        int *__restrict__ err_flag, PotUserArg<USR> pu)
{
  int *sn, *ss;
  long long ti;
  bool valid;
  if(!strict_wave(n, sn, ss, ti, valid))
    return;
  const StrictTarget T = own_target(s_pm, s_type, s_oldacc, wp, ti, valid);
  double pot;
  int nint;
  potential_walk_lane<NG, PM, LATT, USR>(tv, s_pm, s_type, table, wp, utorwpi, reach, valid, T, sn, ss, err_flag, pu, pot, nint);
  if(valid)
    {
      r_pot[ti] = pot;
      r_nint[ti] = nint;
    }
}

// targets: records handed in (ngravs_potential_targets), the columns of k_walk_targets; the sum x G goes to the caller's index
template <int NG, bool PM, bool LATT, bool USR>
__global__ __launch_bounds__(256) void k_potential_targets(TreeView tv, const double4 *__restrict__ s_pm, const unsigned char *__restrict__ s_type,
                                                           const double *__restrict__ table, WalkParams wp, double utorwpi, double reach,
                                                           const double *__restrict__ t_pos, const double *__restrict__ t_oldacc,
                                                           const double *__restrict__ t_mass, const int *__restrict__ t_type,
                                                           const unsigned int *__restrict__ ord, long long nt, double G,
                                                           double *__restrict__ o_pot, int *__restrict__ o_nint, int *__restrict__ err_flag,
                                                           PotUserArg<USR> pu)
{
  int *sn, *ss;
  long long t, me;
  bool valid;
  if(!strict_wave(nt, sn, ss, t, valid))
    return;
  const StrictTarget T = record_target(t_pos, t_oldacc, t_mass, t_type, ord, wp, t, valid, me);
  double pot;
  int nint;
  potential_walk_lane<NG, PM, LATT, USR>(tv, s_pm, s_type, table, wp, utorwpi, reach, valid, T, sn, ss, err_flag, pu, pot, nint);
  if(valid)
    {
      o_pot[me] = pot * G;
      o_nint[me] = nint;
    }
}

// The tail of compute_potential (potential.c:244-337) for one own row, in its order: the self term m / SofteningTable[type] (the
// negative of what the walk added for the row itself: plummer_pot(m, h, 0) = -2.8 m / h, the same operations), the LatticeZero
// term of a comoving periodic run, G, the mesh part, the cosmological term
struct PotTail
{
  double fsoft[NGRAVS_NTYPES];
  int t2g[NGRAVS_NTYPES];
  double lz[NG_MAX];    // LatticeZero[g][g] (Omega0 3 H^2 / (8 pi G))^(1/3), 0 unless comoving and periodic
  double G, rfac;       // rfac: -0.5 Omega0 H^2 (comoving, not periodic) or -0.5 OmegaLambda H^2 (not comoving), else 0
};
// USR: the self term of a type whose species pair [g][g] has an entry is - m pot_spline(1, 1, h, 0, 1) read from the entry's
// table with the walk's own operations (ks: the table per type, -1 without an entry), so that it takes out what the walk added
// for the row itself to the last bit; lz then holds the entries' LatticeZero
struct PotSelf
{
  UserTabs ut;
  int ks[NGRAVS_NTYPES];
};
template <bool USR> using PotSelfArg = std::conditional_t<USR, PotSelf, NoPotUser>;
template <bool USR>
__global__ void k_potential_finish(const double4 *__restrict__ s_pm, const unsigned char *__restrict__ s_type, long long n, PotTail pt,
                                   const double *__restrict__ mesh, double *__restrict__ r_pot, PotSelfArg<USR> ps)
{
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  const double4 p = s_pm[i];
  const int type = s_type[i];
  double pot = r_pot[i];
  const double h_inv = 1 / pt.fsoft[type];
  bool own_table = false;
  if constexpr(USR)
    if(ps.ks[type] >= 0)
      {
        pot -= p.w * ul_spline(ps.ut, ps.ks[type], pt.fsoft[type], 0.0);
        own_table = true;
      }
  if(!own_table)
    pot += p.w * h_inv * 2.8;
  const double lz = pt.lz[pt.t2g[type]];
  if(lz != 0)
    pot -= lz * pow(p.w, 2.0 / 3);
  pot *= pt.G;
  if(mesh)
    pot += mesh[i];
  if(pt.rfac != 0)
    pot += pt.rfac * (p.x * p.x + p.y * p.y + p.z * p.z);
  r_pot[i] = pot;
}

__global__ void k_unpermute_i32(const unsigned int *idx, long long n, const int *src, int *dst)
{
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i < n)
    dst[idx[i]] = src[i];
}

#pragma clang fp contract(fast)

// ---- host side ------------------------------------------------------------------------------------------------------------------
static double law_sign(int law) { return law == NGRAVS_LAW_NEWTON ? 1.0 : (law == NGRAVS_LAW_NEG_NEWTON ? -1.0 : 0.0); }

// the lattice potential tables: one Ewald sum per distinct law, replicated into the [target][source] slots (as ensure_lattice)
int potential_lattice_ensure(ngravs_ctx *c)
{
  if(c->pot_lat_ready)
    return NGRAVS_OK;
  const int ng = c->cfg.n_gravs, npts = LAT_E1 * LAT_E1 * LAT_E1;
  if(c->pot_lat.ensure((size_t)ng * ng * POT_LAT_SZ))
    return NGRAVS_ERR_NOMEM;
  std::vector<double> host;   // one table of the model's (ngravs_create_with_potentials), sampled on the host
  for(int k = 0; k < ng * ng; k++)
    {
      double *dst = c->pot_lat.p + (size_t)k * POT_LAT_SZ;
      if(const ngravs_user_potential_t *e = user_pot_entry(c, k / ng, k % ng))
        {
          // the pair's own LatticePotential and LatticeZero: 65^3 - 1 calls per distinct function and zero
          int src = -1;
          for(int q = 0; q < k && src < 0; q++)
            if(const ngravs_user_potential_t *o = user_pot_entry(c, q / ng, q % ng))
              if(o->lattice_pot == e->lattice_pot && o->lattice_zero == e->lattice_zero)
                src = q;
          if(src >= 0)
            {
              HIP_TRY(c, hipMemcpyAsync(dst, c->pot_lat.p + (size_t)src * POT_LAT_SZ, sizeof(double) * POT_LAT_SZ, hipMemcpyDeviceToDevice, c->stream));
              continue;
            }
          std::string why;
          host.resize(POT_LAT_SZ);
          if(!e->lattice_pot)   // (refused at creation for a periodic tree-only configuration)
            return NGRAVS_ERR_WIRING;
          if(int rc = user_pot_lattice_tabulate(e->lattice_pot, e->lattice_zero, c->cfg.box_size, host.data(), why))
            {
              ngravs_report(c, rc, "potential entry [" + std::to_string(k / ng) + "][" + std::to_string(k % ng) + "]: " + why);
              return rc;
            }
          HIP_TRY(c, hipMemcpyAsync(dst, host.data(), sizeof(double) * POT_LAT_SZ, hipMemcpyHostToDevice, c->stream));
          HIP_TRY(c, hipStreamSynchronize(c->stream));   // (host is reused)
          continue;
        }
      const double sign = law_sign(c->cfg.law_accel[k / ng][k % ng]);
      int src = -1;
      for(int q = 0; q < k && src < 0; q++)
        if(!user_pot_entry(c, q / ng, q % ng) && law_sign(c->cfg.law_accel[q / ng][q % ng]) == sign)
          src = q;
      if(src >= 0)
        HIP_TRY(c, hipMemcpyAsync(dst, c->pot_lat.p + (size_t)src * POT_LAT_SZ, sizeof(double) * POT_LAT_SZ, hipMemcpyDeviceToDevice, c->stream));
      else
        hipLaunchKernelGGL(k_lattice_pot_table, dim3((npts + 63) / 64), dim3(64), 0, c->stream, sign, c->cfg.box_size, dst);
    }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  c->pot_lat_ready = true;
  return NGRAVS_OK;
}

// E[i] = (force_tab[i] + pot_tab[i]) u_i = tempI(u_i) / u_i, the long-range potential of the split (pi erf(u) / u for Newton)
static int potential_table_ensure(ngravs_ctx *c)
{
  if(c->pot_table_ready)
    return NGRAVS_OK;
  const int ng = c->cfg.n_gravs;
  const size_t len = (size_t)ng * ng * NTAB;
  std::vector<double> f(len), p(len);
  host_shortrange_table(&c->cfg, f.data(), p.data(), c->user_fns.data(), (int)c->user_fns.size());
  for(size_t k = 0; k < len; k++)
    f[k] = (f[k] + p[k]) * (3.0 / NTAB * ((double)(k % NTAB) + 0.5));
  if(c->pot_table.ensure(len))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipMemcpyAsync(c->pot_table.p, f.data(), sizeof(double) * len, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->pot_table_ready = true;
  return NGRAVS_OK;
}

// k_potential_walk / k_potential_targets<NG, PM, LATT, USR>: TreePM, periodic tree-only, tree-only; each with the built-in
// companions alone and with the model's tables
template <int NG> using PotRowsNG = Table<Row<NG, 1, 0, 0>, Row<NG, 0, 1, 0>, Row<NG, 0, 0, 0>, Row<NG, 1, 0, 1>, Row<NG, 0, 1, 1>, Row<NG, 0, 0, 1>>;
using PotRows = decltype(PotRowsNG<1>{} + PotRowsNG<2>{} + PotRowsNG<3>{});

struct PotWalk
{
  WalkParams wp;
  double utorwpi, reach;   // 1 / (2 pi Asmth); NTAB / asmthfac = 6 Asmth: tab < NTAB inside it
  const double *table;
  int key[4];
  int *flag;
  PotUser pu;              // USR (key[3]): the model's tables
};
template <bool USR> static PotUserArg<USR> pot_user_arg(const PotWalk &w)
{
  if constexpr(USR)
    return w.pu;
  else
    return NoPotUser{0};
}
// tables, parameters and the zeroed flag word of one potential walk; far: the largest distance of a target from the domain's centre
static int potential_walk_setup(ngravs_ctx *c, PotWalk *w, double far)
{
  const bool pm = c->cfg.pmgrid != 0, latt = c->cfg.periodic && !pm, usr = !c->user_pot.empty();
  int rc;
  if(pm && (rc = potential_table_ensure(c)))
    return rc;
  if(latt && (rc = potential_lattice_ensure(c)))
    return rc;
  if(usr && (rc = user_pot_tables_ensure(c, table_reach(c, true, far))))
    return rc;
  memset(&w->pu, 0, sizeof(w->pu));
  if(usr)
    user_pot_maps(c, &w->pu);
  make_walk_params(c, &w->wp);
  w->utorwpi = pm ? 1.0 / (2 * M_PI * c->asmth) : 0.0;
  w->reach = pm ? NTAB / w->wp.asmthfac : 0.0;
  w->table = pm ? c->pot_table.p : (latt ? c->pot_lat.p : nullptr);
  w->key[0] = c->cfg.n_gravs, w->key[1] = pm, w->key[2] = latt, w->key[3] = usr;
  if(c->gt_counters.ensure(GT_C_COUNT))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipMemsetAsync(c->gt_counters.p, 0, GT_C_COUNT * sizeof(unsigned long long), c->stream));
  w->flag = reinterpret_cast<int *>(c->gt_counters.p + GT_C_FLAG);
  return NGRAVS_OK;
}
static int potential_walk_flag(ngravs_ctx *c, const PotWalk &w)
{
  int flag = 0;
  HIP_TRY(c, hipMemcpyAsync(&flag, w.flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if(flag & 4)
    {
      ngravs_report(c, NGRAVS_ERR_STATE, "the potential walk met a top-level cell whose particles are not on this task");
      return NGRAVS_ERR_STATE;
    }
  return NGRAVS_OK;
}

template <int NG, int PM, int LATT, int USR>
static int launch_potential(Row<NG, PM, LATT, USR>, ngravs_ctx *c, const PotWalk &w, long long n, int *d_nint)
{
  hipLaunchKernelGGL((k_potential_walk<NG, PM, LATT, USR>), strict_grid(n), dim3(256), 0, c->stream, tree_view(c), c->s_pm.p,
                     c->s_type.p, c->s_oldacc.p, w.table, w.wp, w.utorwpi, w.reach, n, c->r_pot.p, d_nint, w.flag, pot_user_arg<USR>(w));
  return NGRAVS_OK;
}
template <int NG, int PM, int LATT, int USR>
static int launch_potential_targets(Row<NG, PM, LATT, USR>, ngravs_ctx *c, const PotWalk &w, long long nt, const unsigned int *ord)
{
  hipLaunchKernelGGL((k_potential_targets<NG, PM, LATT, USR>), strict_grid(nt), dim3(256), 0, c->stream, tree_view(c), c->s_pm.p,
                     c->s_type.p, w.table, w.wp, w.utorwpi, w.reach, c->gt_in.p, c->gt_in.p + 3 * nt, c->gt_in.p + 4 * nt, c->gt_type.p, ord, nt, c->cfg.G,
                     c->gt_acc.p, c->gt_nint.p, w.flag, pot_user_arg<USR>(w));
  return NGRAVS_OK;
}

int potential_run(ngravs_ctx *c, const ngravs_time_params_t *par, double *d_out, int *d_nint)
{
  const long long n = c->n;
  const bool pm = c->cfg.pmgrid != 0;
  // r_pot: the walk's column, behind it the mesh column; gt_nint: the counts in Peano order
  if(c->r_pot.ensure(2 * (size_t)n) || c->gt_nint.ensure((size_t)n))
    return NGRAVS_ERR_NOMEM;
  PotWalk w;
  int rc;
  if((rc = potential_walk_setup(c, &w, 0.0)))   // (own rows: inside the domain)
    return rc;
  HIP_TRY(c, hipEventRecord(c->evk0, c->stream));
  if((rc = dispatch(c, PotRows{}, w.key, [&](auto row) { return launch_potential(row, c, w, n, c->gt_nint.p); })))
    return rc;
  HIP_TRY(c, hipEventRecord(c->evk1, c->stream));
  HIP_TRY(c, hipGetLastError());
  double *mesh = nullptr;
  if(pm)
    {
      // the mesh at the CURRENT positions: deposit, transforms and Green multiply of a PM step, without its force and without
      // touching r_pm or have_pm; pm_phi is then no longer the last PM step's
      if((rc = pm_deposit(c)) || (rc = pm_solve(c)))
        return rc;
      mesh = c->r_pot.p + n;
      HIP_TRY(c, hipMemsetAsync(mesh, 0, sizeof(double) * n, c->stream));
      if((rc = pm_potential_gather(c, nullptr, nullptr, n, mesh)))
        return rc;
      c->pot_mesh_valid = true;
    }
  PotTail pt;
  memset(&pt, 0, sizeof(pt));
  for(int t = 0; t < NGRAVS_NTYPES; t++)
    {
      pt.fsoft[t] = c->cfg.force_softening[t];
      pt.t2g[t] = c->cfg.type_to_grav[t];
    }
  pt.G = c->cfg.G;
  if(par && par->comoving)
    {
      if(c->cfg.periodic)
        for(int g = 0; g < c->cfg.n_gravs; g++)
          {
            const ngravs_user_potential_t *e = user_pot_entry(c, g, g);   // the model's LatticeZero[g][g]
            pt.lz[g] = (e ? e->lattice_zero : law_sign(c->cfg.law_accel[g][g]) * LATTICE_ZERO) *
                       pow(par->omega0 * 3 * par->hubble * par->hubble / (8 * M_PI * c->cfg.G), 1.0 / 3);   // potential.c:256-257
          }
      else
        pt.rfac = -0.5 * par->omega0 * par->hubble * par->hubble;                                         // potential.c:313
    }
  else if(par)
    pt.rfac = -0.5 * par->omega_lambda * par->hubble * par->hubble;                                       // potential.c:326
  if(w.key[3])
    {
      PotSelf ps;
      ps.ut = w.pu.ut;
      for(int t = 0; t < NGRAVS_NTYPES; t++)
        ps.ks[t] = w.pu.ks[pt.t2g[t]][pt.t2g[t]];
      hipLaunchKernelGGL(k_potential_finish<true>, GRID1(n), 0, c->stream, c->s_pm.p, c->s_type.p, n, pt, mesh, c->r_pot.p, ps);
    }
  else
    hipLaunchKernelGGL(k_potential_finish<false>, GRID1(n), 0, c->stream, c->s_pm.p, c->s_type.p, n, pt, mesh, c->r_pot.p, NoPotUser{0});
  hipLaunchKernelGGL(k_unpermute_f64, GRID1(n), 0, c->stream, c->s_idx.p, n, 1, c->r_pot.p, d_out);
  if(d_nint)
    hipLaunchKernelGGL(k_unpermute_i32, GRID1(n), 0, c->stream, c->s_idx.p, n, c->gt_nint.p, d_nint);
  HIP_TRY(c, hipGetLastError());
  if((rc = potential_walk_flag(c, w)))
    return rc;
  float ms = 0;
  (void)hipEventElapsedTime(&ms, c->evk0, c->evk1);   // (complete: potential_walk_flag waited for the stream)
  c->pot_walk_ms = ms;
  return NGRAVS_OK;
}

int potential_targets_run(ngravs_ctx *c, long long nt, double far)
{
  if(c->gt_acc.ensure(3 * (size_t)nt) || c->gt_nint.ensure((size_t)nt))
    return NGRAVS_ERR_NOMEM;
  PotWalk w;
  int rc;
  if((rc = potential_walk_setup(c, &w, far)))
    return rc;
  const unsigned int *ord;
  if((rc = grav_targets_order(c, nt, &ord)))
    return rc;
  if((rc = dispatch(c, PotRows{}, w.key, [&](auto row) { return launch_potential_targets(row, c, w, nt, ord); })))
    return rc;
  HIP_TRY(c, hipGetLastError());
  if(c->cfg.pmgrid && (rc = pm_potential_gather(c, c->gt_in.p, c->gt_type.p, nt, c->gt_acc.p)))
    return rc;
  return potential_walk_flag(c, w);
}
