/* tests/glue_stub_sph/glue_sph_driver.c -- TEST-ONLY: a one-task stand-in for the units that stay around gadget_glue.c in a gas run
 * (-DNGRAVS_GLUE_SPH), so that the glue's density(), hydro_force() and ngb_tree*() are RUN on the GPU in the reference's own order:
 *
 *   stage 0, init() (init.c:140-175): SphP[].Hsml = 0, ngb_treeallocate(), force_treeallocate(), domain_Decomposition(),
 *            ngb_treebuild(), the host loop of setup_smoothinglengths() over Father[] / Nodes[] (restated below; it must leave
 *            Hsml = 0 and change nothing else), density(), the conversion of internal energy to entropy (init.c:170-174);
 *   stage 1, a first step, every particle active (run.c, accel.c:24-96): domain_Decomposition(), [pmforce_periodic()],
 *            gravity_tree(), density(), force_update_hmax(), hydro_force();
 *   stage 2, a second step that keeps decomposition and tree (domain.c:76): drifted positions, one gas particle in three active,
 *            Ti_begstep / Ti_endstep on two rungs, the DtEntropy of stage 1 in the pressure line.
 *
 * After every stage the run's state goes to the output file: a header of 12 doubles (stage, NumPart, N_gas, the four SPH timers,
 * three flags, 2 spare), SphP[0..N_gas) as it lies in memory (21 doubles a row), and 9 doubles for every row of P[] (GravAccel,
 * OldAcc, GravCost, Ti_begstep, Ti_endstep, Type, ID).  With gas_calls = 0 in the input the three SPH calls of stages 1 and 2 are
 * left out (what gravity gives without them).
 *
 *   gcc -DNGRAVS_BUILD_INSIDE_REFERENCE -DDOUBLEPRECISION -DUNEQUALSOFTENINGS -DNGRAVS_GLUE_SPH -DN_GRAVS=1 [-DPERIODIC -DPMGRID=32]
 *       -Itests/glue_stub_sph -Itests/glue_stub -Iinclude host/gadget_glue.c tests/glue_stub_sph/glue_sph_driver.c -lngravs_hip -lm
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <time.h>
#include <unistd.h>
#include <mpi.h>
#include "allvars.h"
#include "proto.h"
#include "ngravs.h"

#define MAX_NGB 20000		/* allvars.h:91 */

/* ---- allvars.c ----------------------------------------------------------------------------------------------------------- */
gravity AccelFxns[N_GRAVS][N_GRAVS], AccelSplines[N_GRAVS][N_GRAVS], GreensFxns[N_GRAVS][N_GRAVS], NormedGreensFxns[N_GRAVS][N_GRAVS];
int TypeToGrav[6];
int NgravLocal[N_GRAVS];
int ThisTask = 0, NTask = 1, NumPart = 0;
int N_gas = 0;
int RestartFlag = 0;
int *Ngblist;
long long Ntype[6];
int NtypeLocal[6];
int TreeReconstructFlag;
double DomainCorner[3], DomainCenter[3], DomainLen, DomainFac;
double TimeOfLastTreeConstruction;
FILE *FdTimings, *FdForceTest;
int Numnodestree;
int *Father;
struct global_data_all_processes All;
struct particle_data *P;
struct sph_particle_data *SphP;
struct NODE *Nodes;

/* ---- force laws: only their addresses are used here ------------------------------------------------------------------------ */
#define LAWBODY(f) double f(double a, double b, double c, double d, long n) { (void)a; (void)b; (void)c; (void)d; (void)n; return 0.0; }
LAWBODY(none) LAWBODY(newtonian) LAWBODY(neg_newtonian) LAWBODY(plummer) LAWBODY(neg_plummer) LAWBODY(pgdelta) LAWBODY(neg_pgdelta)
LAWBODY(normed_pgdelta) LAWBODY(bambam) LAWBODY(sourcebambaryon) LAWBODY(sourcebaryonbam) LAWBODY(bambam_spline)
LAWBODY(sourcebambaryon_spline) LAWBODY(sourcebaryonbam_spline) LAWBODY(yukawa) LAWBODY(pgyukawa) LAWBODY(normed_pgyukawa)
LAWBODY(coloyuk) LAWBODY(pgcoloyuk) LAWBODY(normed_pgcoloyuk)

/* ---- system.c / run.c helpers ------------------------------------------------------------------------------------------------ */
double second(void)
{
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
double timediff(double t0, double t1) { return t1 - t0; }
void endrun(int code)
{
  printf("task %d: endrun(%d)\n", ThisTask, code);
  fflush(stdout);
  _exit(code ? (code & 127) | 1 : 0);
}
double get_random_number(int id)
{
  unsigned int x = (unsigned int)id * 2654435761u;
  x ^= x >> 15;
  return (double)(x % 1000u) / 1000.0;
}
#ifdef PERIODIC
void do_box_wrapping(void)   /* predict.c:107-133 */
{
  int i, j;
  for(i = 0; i < NumPart; i++)
    for(j = 0; j < 3; j++)
      {
        while(P[i].Pos[j] < 0)
          P[i].Pos[j] += All.BoxSize;
        while(P[i].Pos[j] >= All.BoxSize)
          P[i].Pos[j] -= All.BoxSize;
      }
}
#endif

/* ---- MPI with one task: every collective is a copy ----------------------------------------------------------------------------- */
static size_t tsize(MPI_Datatype t) { return t == MPI_BYTE ? 1 : (t == MPI_INT ? 4 : 8); }
int MPI_Allreduce(const void *s, void *r, int n, MPI_Datatype t, MPI_Op o, MPI_Comm c)
{
  (void)o;
  (void)c;
  if(s != MPI_IN_PLACE)
    memcpy(r, s, tsize(t) * (size_t)n);
  return MPI_SUCCESS;
}
int MPI_Barrier(MPI_Comm c)
{
  (void)c;
  return MPI_SUCCESS;
}
int MPI_Allgatherv(const void *s, int n, MPI_Datatype t, void *r, const int *cnt, const int *dsp, MPI_Datatype rt, MPI_Comm c)
{
  (void)cnt;
  (void)rt;
  (void)c;
  memcpy((char *)r + tsize(t) * (size_t)dsp[0], s, tsize(t) * (size_t)n);
  return MPI_SUCCESS;
}
int MPI_Bcast(void *b, int n, MPI_Datatype t, int root, MPI_Comm c)
{
  (void)b;
  (void)n;
  (void)t;
  (void)root;
  (void)c;
  return MPI_SUCCESS;
}
int MPI_Allgather(const void *s, int n, MPI_Datatype t, void *r, int rn, MPI_Datatype rt, MPI_Comm c)
{
  (void)rn;
  (void)rt;
  (void)c;
  memcpy(r, s, tsize(t) * (size_t)n);
  return MPI_SUCCESS;
}
int MPI_Alltoall(const void *s, int n, MPI_Datatype t, void *r, int rn, MPI_Datatype rt, MPI_Comm c)
{
  (void)rn;
  (void)rt;
  (void)c;
  memcpy(r, s, tsize(t) * (size_t)n);
  return MPI_SUCCESS;
}
int MPI_Alltoallv(const void *s, const int *sc, const int *sd, MPI_Datatype t, void *r, const int *rc, const int *rd, MPI_Datatype rt, MPI_Comm c)
{
  (void)rc;
  (void)rt;
  (void)c;
  if(sc[0] > 0)
    memcpy((char *)r + tsize(t) * (size_t)rd[0], (const char *)s + tsize(t) * (size_t)sd[0], tsize(t) * (size_t)sc[0]);
  return MPI_SUCCESS;
}
/* one task sends nothing to itself through the glue's all-to-all-v (its counts for the own rank are 0) */
int MPI_Irecv(void *b, int n, MPI_Datatype t, int src, int tag, MPI_Comm c, MPI_Request *q)
{
  (void)b;
  (void)n;
  (void)t;
  (void)src;
  (void)tag;
  (void)c;
  *q = 0;
  return 1;
}
int MPI_Isend(const void *b, int n, MPI_Datatype t, int dst, int tag, MPI_Comm c, MPI_Request *q)
{
  (void)b;
  (void)n;
  (void)t;
  (void)dst;
  (void)tag;
  (void)c;
  *q = 0;
  return 1;
}
int MPI_Waitall(int n, MPI_Request *q, MPI_Status *s)
{
  (void)n;
  (void)q;
  (void)s;
  return MPI_SUCCESS;
}

/* ---- the run ----------------------------------------------------------------------------------------------------------------- */
static int HostLoopOk = 0;	/* the loop of setup_smoothinglengths() left Hsml = 0 in every gas row and Father / the node as allocated */

/* Father[] and the one host node as force_treeallocate() wrote them (before the first density()), or Father[] = -1 (after it);
 * the node itself is never written */
static int father_all(int value)
{
  int i;
  for(i = 0; i < All.MaxPart; i++)
    if(Father[i] != value)
      return 0;
  return 1;
}
static int node_untouched(void)
{
  const struct NODE *nd = &Nodes[All.MaxPart];
  int k, ok = nd->len == 0 && nd->u.d.father == -1;
  for(k = 0; k < N_GRAVS; k++)
    ok = ok && nd->u.d.mass[k] == 1;
  return ok;
}

static void dump(FILE *f, int stage)
{
  double hd[12] = {(double)stage, (double)NumPart, (double)N_gas, All.CPU_HydCompWalk, All.CPU_HydCommSumm, All.CPU_HydImbalance,
    All.CPU_EnsureNgb, (double)father_all(-1), (double)node_untouched(), (double)HostLoopOk, 0, 0
  };
  int i;
  fwrite(hd, sizeof(double), 12, f);
  fwrite(SphP, sizeof(struct sph_particle_data), (size_t)N_gas, f);
  for(i = 0; i < NumPart; i++)
    {
      double row[9] = {P[i].GravAccel[0], P[i].GravAccel[1], P[i].GravAccel[2], P[i].OldAcc, (double)P[i].GravCost, (double)P[i].Ti_begstep,
	(double)P[i].Ti_endstep, (double)P[i].Type, (double)P[i].ID
      };
      fwrite(row, sizeof(double), 9, f);
    }
}

int main(int argc, char **argv)
{
  FILE *f;
  double hd[20];
  int i, j, n, gas_calls;
  if(argc < 3)
    return 2;
  if(sizeof(struct sph_particle_data) != 21 * sizeof(double))
    return 6;
  if(!(f = fopen(argv[1], "rb")))
    return 2;
  /* header: n, n_gas, gas_calls, G, BoxSize, ErrTolTheta, ErrTolForceAcc, DesNumNgb, MaxNumNgbDeviation, ArtBulkViscConst,
   * Timebase_interval, softening[6] */
  if(fread(hd, sizeof(double), 17, f) != 17)
    return 3;
  n = (int)hd[0];
  N_gas = (int)hd[1];
  gas_calls = (int)hd[2];
  memset(&All, 0, sizeof(All));
  All.G = hd[3];
  All.BoxSize = hd[4];
  All.ErrTolTheta = hd[5];
  All.ErrTolForceAcc = hd[6];
  All.DesNumNgb = hd[7];
  All.MaxNumNgbDeviation = hd[8];
  All.ArtBulkViscConst = hd[9];
  All.Timebase_interval = hd[10];
  All.SofteningGas = hd[11];
  All.SofteningHalo = hd[12];
  All.SofteningDisk = hd[13];
  All.SofteningBulge = hd[14];
  All.SofteningStars = hd[15];
  All.SofteningBndry = hd[16];
  All.TypeOfOpeningCriterion = 0;	/* Barnes-Hut throughout: the walk does not depend on OldAcc, two runs open the same nodes */
  All.TotNumPart = n;
  All.TotN_gas = N_gas;
  All.PartAllocFactor = 1.6;
  All.MaxPart = (int)(All.PartAllocFactor * n) + 16;
  All.TreeAllocFactor = 0.8;
  All.TreeDomainUpdateFrequency = 0.0;
  All.Time = 1.0;
  All.MinGasHsmlFractional = 0.0;
  strcpy(All.OutputDir, argc > 3 ? argv[3] : "./");
  P = calloc((size_t)All.MaxPart, sizeof(*P));
  SphP = calloc((size_t)(N_gas > 0 ? N_gas : 1), sizeof(*SphP));	/* N_gas rows and not one more: nothing may read behind them */
  /* rows: Pos[3], Mass, Type, Vel[3], internal energy (gas rows first, the reference's order after read_ic()) */
  for(i = 0; i < n; i++)
    {
      double row[9];
      if(fread(row, sizeof(double), 9, f) != 9)
        return 4;
      for(j = 0; j < 3; j++)
        {
          P[i].Pos[j] = row[j];
          P[i].Vel[j] = row[5 + j];
        }
      P[i].Mass = row[3];
      P[i].Type = (int)row[4];
      P[i].ID = (unsigned int)(i + 1);
      if(i < N_gas)
        {
          SphP[i].Entropy = row[8];	/* the internal energy, until init() converts it */
          for(j = 0; j < 3; j++)
            SphP[i].VelPred[j] = P[i].Vel[j];	/* init.c:127-128 */
          SphP[i].Hsml = 0;	/* init.c:144 */
        }
    }
  NumPart = n;
  fclose(f);
  for(i = 0; i < 6; i++)
    TypeToGrav[i] = (i >= 1 && i <= N_GRAVS) ? i - 1 : 0;
  for(i = 0; i < N_GRAVS; i++)
    for(j = 0; j < N_GRAVS; j++)
      {
        const int cross = i != j;
        AccelFxns[i][j] = cross ? coloyuk : newtonian;
        AccelSplines[i][j] = plummer;
        GreensFxns[i][j] = cross ? pgcoloyuk : pgdelta;
        NormedGreensFxns[i][j] = cross ? normed_pgcoloyuk : normed_pgdelta;
      }
  {
    char tn[600];
    snprintf(tn, sizeof(tn), "%stimings.txt", argc > 3 ? argv[3] : "/tmp/");
    FdTimings = fopen(tn, "w");
  }
  if(!(f = fopen(argv[2], "wb")) || !FdTimings)
    return 5;

  /* ---- stage 0: init() ---- */
  set_softenings();		/* init.c:60 */
#ifdef PMGRID
  pm_init_periodic();
#endif
#ifdef PERIODIC
  lattice_init();
#endif
  All.Ti_Current = 0;
  All.PM_Ti_endstep = 0;
  ngb_treeallocate(MAX_NGB);	/* init.c:149 */
  force_treeallocate((int)(All.TreeAllocFactor * All.MaxPart), All.MaxPart);	/* init.c:151 */
  All.NumForcesSinceLastDomainDecomp = 1 + All.TotNumPart * All.TreeDomainUpdateFrequency;
  domain_Decomposition();	/* init.c:157 */
  ngb_treebuild();		/* init.c:159 */
  {
    /* setup_smoothinglengths(), init.c:229-247, in this driver's words: climb from Father[i] while the node is too light */
    const int was_on_node = father_all(All.MaxPart);
    int ok = 1;
    for(i = 0; i < N_gas; i++)
      {
        int no = Father[i];
        while(10 * All.DesNumNgb * P[i].Mass > Nodes[no].u.d.mass[TypeToGrav[0]])
          {
            const int up = Nodes[no].u.d.father;
            if(up < 0)
              break;
            no = up;
          }
        SphP[i].Hsml = pow(3.0 / (4 * M_PI) * All.DesNumNgb * P[i].Mass / Nodes[no].u.d.mass[TypeToGrav[0]], 1.0 / 3) * Nodes[no].len;
        ok = ok && SphP[i].Hsml == 0;
      }
    HostLoopOk = ok && was_on_node && father_all(All.MaxPart) && node_untouched();
  }
  density();			/* init.c:255 */
#ifndef ISOTHERM_EQS
  for(i = 0; i < N_gas; i++)	/* init.c:170-174 (a3 = 1: no comoving integration) */
    SphP[i].Entropy = GAMMA_MINUS1 * SphP[i].Entropy / pow(SphP[i].Density / 1.0, GAMMA_MINUS1);
#endif
  dump(f, 0);

  /* ---- stage 1: the first step, everything active ---- */
  domain_Decomposition();	/* run.c:68 (NumForcesSinceLastDomainDecomp is still above the limit: decomposes and rebuilds) */
#ifdef PMGRID
  pmforce_periodic();
#endif
  gravity_tree();
  if(gas_calls)
    {
      density();
      force_update_hmax();
      hydro_force();
    }
  dump(f, 1);

  /* ---- stage 2: a step that keeps decomposition and tree; drifted positions, one gas particle in three active ---- */
  All.TreeDomainUpdateFrequency = 1.0;
  All.NumForcesSinceLastDomainDecomp = 0;
  All.Ti_Current = 8;
  All.PM_Ti_endstep = 16;
  for(i = 0; i < NumPart; i++)
    {
      const int id = (int)P[i].ID - 1;
      if(id % 3 == 1)		/* active, on two rungs */
        {
          P[i].Ti_begstep = (id % 2) ? 4 : 0;
          P[i].Ti_endstep = 8;
        }
      else
        {
          P[i].Ti_begstep = (id % 2) ? 4 : 0;
          P[i].Ti_endstep = (id % 2) ? 12 : 16;
        }
      for(j = 0; j < 3; j++)
        P[i].Pos[j] += 1e-3 * (All.BoxSize > 0 ? All.BoxSize : 1.0) * sin(0.37 * (double)P[i].ID + 1.3 * j);
    }
  domain_Decomposition();
  gravity_tree();
  if(gas_calls)
    {
      density();
      force_update_hmax();
      hydro_force();
    }
  dump(f, 2);
  fclose(f);
  ngb_treefree();
  force_treefree();
  printf("glue sph driver: %d particles, %d gas, three stages done\n", NumPart, N_gas);
  return 0;
}
