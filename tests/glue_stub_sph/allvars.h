/* tests/glue_stub_sph/allvars.h -- TEST-ONLY declarations of the reference globals gadget_glue.c touches when it is built with
 * -DNGRAVS_GLUE_SPH (a gas run): everything tests/glue_stub/allvars.h declares, plus GAMMA (allvars.h:49-55), struct
 * sph_particle_data (allvars.h:587-605, every field, the reference's order), the fields of struct NODE the kept init.c reads
 * (allvars.h:618-659), N_gas, RestartFlag, Ngblist and the All fields of the SPH path.  tools/glue_stub_check.py --sph holds them to
 * the reference's headers (tests/golden/glue_stub_sph_check.json).  Nothing here is used by the product. */
#ifndef ALLVARS_H
#define ALLVARS_H
#include <stdio.h>
#ifndef N_GRAVS
#define N_GRAVS 2
#endif
#define ASMTH 1.25
#define RCUT 4.5
#define MAXLEN_FILENAME 100
#ifdef DOUBLEPRECISION
#define FLOAT double
#else
#define FLOAT float
#endif
#ifdef ISOTHERM_EQS
#define GAMMA (1.0)
#else
#define GAMMA (5.0/3)
#endif
#define GAMMA_MINUS1 (GAMMA-1)
typedef long long peanokey;
typedef double (*gravity)(double, double, double, double, long);

extern gravity AccelFxns[N_GRAVS][N_GRAVS], AccelSplines[N_GRAVS][N_GRAVS], GreensFxns[N_GRAVS][N_GRAVS], NormedGreensFxns[N_GRAVS][N_GRAVS];
extern int TypeToGrav[6];
extern int NgravLocal[N_GRAVS];
extern int ThisTask, NTask, NumPart;
extern int N_gas;
extern int RestartFlag;
extern int *Ngblist;
extern long long Ntype[6];
extern int NtypeLocal[6];
extern int TreeReconstructFlag;
extern double DomainCorner[3], DomainCenter[3], DomainLen, DomainFac;
extern double TimeOfLastTreeConstruction;
extern FILE *FdTimings, *FdForceTest;
extern int Numnodestree;
extern int *Father;

extern struct global_data_all_processes
{
  long long TotNumPart, TotN_gas;
  int MaxPart;
  double PartAllocFactor, TreeAllocFactor;
  double ErrTolTheta, ErrTolForceAcc;
  int TypeOfOpeningCriterion;
  long long TotNumOfForces, NumForcesSinceLastDomainDecomp;
  double G, BoxSize, Time, TimeStep;
  int NumCurrentTiStep, Ti_Current, PM_Ti_endstep;
  double Asmth[2], Rcut[2];
  double ForceSoftening[6], SofteningTable[6];
  double SofteningGas, SofteningHalo, SofteningDisk, SofteningBulge, SofteningStars, SofteningBndry;
  double SofteningGasMaxPhys, SofteningHaloMaxPhys, SofteningDiskMaxPhys, SofteningBulgeMaxPhys, SofteningStarsMaxPhys, SofteningBndryMaxPhys;
  double MinGasHsml, MinGasHsmlFractional;
  double DesNumNgb, MaxNumNgbDeviation, ArtBulkViscConst;
  double Timebase_interval;
  double Hubble, Omega0, OmegaLambda;
  double CPU_HydCompWalk, CPU_HydCommSumm, CPU_HydImbalance, CPU_EnsureNgb;
  int ComovingIntegrationOn;
  double TreeDomainUpdateFrequency;
  double CPU_TreeConstruction, CPU_TreeWalk, CPU_Imbalance, CPU_CommSum, CPU_PM, CPU_Domain, CPU_Peano;
  char OutputDir[MAXLEN_FILENAME];
} All;

extern struct particle_data
{
  FLOAT Pos[3], Mass, Vel[3], GravAccel[3];
#ifdef PMGRID
  FLOAT GravPM[3];
#endif
#ifdef FORCETEST
  FLOAT GravAccelDirect[3];
#endif
  FLOAT Potential, OldAcc;
  unsigned int ID;
  int Type, Ti_endstep, Ti_begstep;
  float GravCost;
} *P;

extern struct sph_particle_data
{
  FLOAT Entropy;
  FLOAT Density;
  FLOAT Hsml;
  FLOAT Left;
  FLOAT Right;
  FLOAT NumNgb;
  FLOAT Pressure;
  FLOAT DtEntropy;
  FLOAT HydroAccel[3];
  FLOAT VelPred[3];
  FLOAT DivVel;
  FLOAT CurlVel;
  FLOAT Rot[3];
  FLOAT DhsmlDensityFactor;
  FLOAT MaxSignalVel;
} *SphP;

/* only what setup_smoothinglengths() (init.c:231-247) and the node loop of timestep.c:333-343 read */
extern struct NODE
{
  FLOAT len;
  union
  {
    struct
    {
      FLOAT s[3][N_GRAVS];
      FLOAT mass[N_GRAVS];
      int father;
    }
    d;
  }
  u;
} *Nodes;
#endif
