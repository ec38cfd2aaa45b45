/* Single-task driver for the reference's own SPH path: reads one binary input file, fills the reference's globals, calls the
 * reference's domain_Decomposition(), ngb_treebuild(), density(), force_update_hmax(), hydro_force() and writes the SphP
 * columns of every gas particle.  The project's own text: it holds no numerics of the reference and is compiled against the
 * reference's headers in place (see Makefile, target ref).  Front end: ref_sph.py.
 *
 * input  (native endianness, written by ref_sph.py):
 *   char magic[8] = "NGSPHIN1"
 *   int32  mode (0: density() then hydro_force(); 1: hydro_force() alone on the given SphP columns), n, comoving, ti_current, buffer_mb
 *   double box_size, des_num_ngb, max_num_ngb_deviation, min_gas_hsml, art_bulk_visc_const, timebase_interval, time, omega0,
 *          omega_lambda, hubble, part_alloc_factor, tree_alloc_factor, force_softening
 *   per particle, in the caller's row order, one array after the other:
 *   double pos[n][3], mass[n]; int32 type[n]; double vel_pred[n][3], hsml[n], entropy[n]; int32 ti_begstep[n], ti_endstep[n]
 *   mode 1 only: double density[n], pressure[n], dhsml_factor[n], div_vel[n], curl_vel[n]
 *   (SphP columns of rows that are not gas are read and dropped)
 * output:
 *   char magic[8] = "NGSPHOU1"; int32 n_gas; int32 row[n_gas]; then 14 arrays double[n_gas] in the order of OUT_NAMES of ref_sph.py
 * The particle ID is the caller's row, so results are mapped back whatever the reference does to the particle order. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <mpi.h>

#include "allvars.h"
#include "proto.h"

static void die(const char *what)
{
  fflush(stdout);
  fprintf(stderr, "ref_sph_driver: %s\n", what);
  exit(2);
}

static void *get(FILE *f, size_t bytes)
{
  void *p = malloc(bytes ? bytes : 1);
  if(!p || fread(p, 1, bytes, f) != bytes)
    die("short input file");
  return p;
}

#ifdef PERIODIC
/* The reference wraps positions into the box in predict.c, which also holds the drift (GSL integration) and is not
 * built here.  The driver's contract is that positions arrive inside [0, BoxSize): wrapping is then the identity. */
void do_box_wrapping(void)
{
  int i, k;
  for(i = 0; i < NumPart; i++)
    for(k = 0; k < 3; k++)
      if(!(P[i].Pos[k] >= 0 && P[i].Pos[k] < All.BoxSize))
        die("a position outside [0, BoxSize) in a periodic run");
}
#endif

int main(int argc, char **argv)
{
  FILE *f;
  char magic[8];
  int head[5], n, i, k, m, ngas, mode;
  double par[13];
  double *pos, *mass, *vel, *hsml, *entropy, *sph[5] = { 0, 0, 0, 0, 0 };
  int *type, *beg, *end, *order;
  unsigned long long lcg = 88172645463325252ULL;

  if(argc != 3)
    die("usage: ref_sph_<variant> INPUT OUTPUT");
  if(!(f = fopen(argv[1], "rb")))
    die("cannot open the input file");
  if(fread(magic, 1, 8, f) != 8 || memcmp(magic, "NGSPHIN1", 8))
    die("not an input file of this driver");
  if(fread(head, sizeof(int), 5, f) != 5 || fread(par, sizeof(double), 13, f) != 13)
    die("short input header");
  mode = head[0];
  n = head[1];
  if(n <= 0 || (mode != 0 && mode != 1))
    die("bad header");
  pos = get(f, sizeof(double) * 3 * n);
  mass = get(f, sizeof(double) * n);
  type = get(f, sizeof(int) * n);
  vel = get(f, sizeof(double) * 3 * n);
  hsml = get(f, sizeof(double) * n);
  entropy = get(f, sizeof(double) * n);
  beg = get(f, sizeof(int) * n);
  end = get(f, sizeof(int) * n);
  if(mode == 1)
    for(k = 0; k < 5; k++)
      sph[k] = get(f, sizeof(double) * n);
  fclose(f);

  /* gas first, as the reference requires */
  order = malloc(sizeof(int) * n);
  for(i = 0, m = 0; i < n; i++)
    if(type[i] == 0)
      order[m++] = i;
  ngas = m;
  for(i = 0; i < n; i++)
    {
      if(type[i] < 0 || type[i] > 5)
        die("particle type outside 0..5");
      if(type[i] != 0)
        order[m++] = i;
    }

  memset(&All, 0, sizeof(All));
  ThisTask = 0;
  NTask = 1;
  PTask = 0;
  NumPart = n;
  N_gas = ngas;
  All.TotNumPart = n;
  All.TotN_gas = ngas;
  All.ComovingIntegrationOn = head[2];
  All.Ti_Current = head[3];
  All.BufferSize = head[4];
  All.BoxSize = par[0];
  All.DesNumNgb = par[1];
  All.MaxNumNgbDeviation = par[2];
  All.MinGasHsml = par[3];
  All.ArtBulkViscConst = par[4];
  All.Timebase_interval = par[5];
  All.Time = par[6];
  All.Omega0 = par[7];
  All.OmegaLambda = par[8];
  All.Hubble = par[9];
  All.PartAllocFactor = par[10];
  All.TreeAllocFactor = par[11];
  for(k = 0; k < 6; k++)
    All.SofteningTable[k] = All.ForceSoftening[k] = par[12];
#ifdef PERIODIC
  All.PeriodicBoundariesOn = 1;
#endif
  All.MaxPart = (int) (All.PartAllocFactor * n);
  All.MaxPartSph = (int) (All.PartAllocFactor * ngas);
  if(All.MaxPart < n || All.MaxPartSph < ngas)
    die("part_alloc_factor below 1");
  for(k = 0; k < 6; k++)
    TypeToGrav[k] = 0;
  /* the table the tree build draws a subnode from when particles coincide: any numbers in [0, 1) serve, they place a
   * particle in the tree and enter no sum (the reference fills it from GSL) */
  for(k = 0; k < RNDTABLE; k++)
    {
      lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
      RndTable[k] = (double) (lcg >> 11) / 9007199254740992.0;
    }

  /* what begrun() / init() would have allocated, by the reference's own allocators */
  allocate_commbuffers();
  allocate_memory();
  ngb_treeallocate(MAX_NGB);
  force_treeallocate((int) (All.TreeAllocFactor * All.MaxPart), All.MaxPart);

  memset(P, 0, sizeof(struct particle_data) * All.MaxPart);
  if(All.MaxPartSph > 0)
    memset(SphP, 0, sizeof(struct sph_particle_data) * All.MaxPartSph);
  for(m = 0; m < n; m++)
    {
      i = order[m];
      for(k = 0; k < 3; k++)
        {
          P[m].Pos[k] = pos[3 * i + k];
          P[m].Vel[k] = vel[3 * i + k];
        }
      P[m].Mass = mass[i];
      P[m].ID = (unsigned int) i;
      P[m].Type = type[i];
      P[m].Ti_begstep = beg[i];
      P[m].Ti_endstep = end[i];
      if(m < ngas)
        {
          for(k = 0; k < 3; k++)
            SphP[m].VelPred[k] = vel[3 * i + k];
          SphP[m].Hsml = hsml[i];
          SphP[m].Entropy = entropy[i];
          if(mode == 1)
            {
              SphP[m].Density = sph[0][i];
              SphP[m].Pressure = sph[1][i];
              SphP[m].DhsmlDensityFactor = sph[2][i];
              SphP[m].DivVel = sph[3][i];
              SphP[m].CurlVel = sph[4][i];
            }
        }
    }

  All.TreeDomainUpdateFrequency = 0;
  All.NumForcesSinceLastDomainDecomp = 1;      /* "it is time for a decomposition" */
  domain_Decomposition();
  ngb_treebuild();
  if(mode == 0)
    {
      density();
      force_update_hmax();
    }
  hydro_force();
  fflush(stdout);

  if(!(f = fopen(argv[2], "wb")))
    die("cannot open the output file");
  fwrite("NGSPHOU1", 1, 8, f);
  fwrite(&ngas, sizeof(int), 1, f);
  for(m = 0; m < ngas; m++)
    {
      int row = (int) P[m].ID;
      if(P[m].Type != 0)
        die("the gas block moved");
      fwrite(&row, sizeof(int), 1, f);
    }
#define PUT(expr) for(m = 0; m < ngas; m++) { double v = (expr); fwrite(&v, sizeof(double), 1, f); }
  PUT(SphP[m].Hsml)
  PUT(SphP[m].Density)
  PUT(SphP[m].NumNgb)
  PUT(SphP[m].DivVel)
  PUT(SphP[m].CurlVel)
  PUT(SphP[m].DhsmlDensityFactor)
  PUT(SphP[m].Pressure)
  PUT(SphP[m].HydroAccel[0])
  PUT(SphP[m].HydroAccel[1])
  PUT(SphP[m].HydroAccel[2])
  PUT(SphP[m].DtEntropy)
  PUT(SphP[m].MaxSignalVel)
  PUT((double) P[m].Ti_begstep)
  PUT((double) P[m].Ti_endstep)
  if(fclose(f))
    die("writing the output file failed");
  return 0;
}
