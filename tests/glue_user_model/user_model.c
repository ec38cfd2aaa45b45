/* A model's own ngravs.c in miniature: copies of newtonian / plummer / pgdelta / normed_pgdelta (ngravs.c:351, :390-402,
 * :420-434) at addresses the glue does not know.  Linked into tests/glue_stub/glue_driver.c with gadget_glue.c built with
 * -Dset_softenings=glue_set_softenings: the driver's set_softenings() call (init.c:60, after init_grav_maps) lands here, re-wires
 * every slot the driver wired with a built-in Newton / Plummer to the copies, and goes on into the glue's own set_softenings. */
#include "allvars.h"
#include "proto.h"
#include "ngravs.h"

void glue_set_softenings(void);

static double model_newtonian(double target, double source, double h, double r, long N)
{
  (void)target;
  (void)r;
  (void)N;
  return source / h;
}
static double model_pgdelta(double target, double source, double k2, double k, long N)
{
  (void)target;
  (void)source;
  (void)k;
  (void)N;
  return 1.0 / k2;
}
static double model_normed_pgdelta(double target, double source, double k2, double k, long N)
{
  (void)target;
  (void)source;
  (void)k2;
  (void)k;
  (void)N;
  return 1.0;
}
static double model_plummer(double target, double source, double h, double r, long N)
{
  double h_inv = 1 / h;

  (void)target;
  (void)N;
  r *= h_inv;
  if(r < 0.5)
    return source * h_inv * h_inv * h_inv * (10.666666666667 + r * r * (32.0 * r - 38.4));
  return source * h_inv * h_inv * h_inv *
         (21.333333333333 - 48.0 * r + 38.4 * r * r - 10.666666666667 * r * r * r - 0.066666666667 / (r * r * r));
}

void set_softenings(void)
{
  int i, j;

  for(i = 0; i < N_GRAVS; i++)
    for(j = 0; j < N_GRAVS; j++)
      {
        if(AccelFxns[i][j] == newtonian)
          AccelFxns[i][j] = model_newtonian;
        if(AccelSplines[i][j] == plummer)
          AccelSplines[i][j] = model_plummer;
        if(GreensFxns[i][j] == pgdelta)
          GreensFxns[i][j] = model_pgdelta;
        if(NormedGreensFxns[i][j] == normed_pgdelta)
          NormedGreensFxns[i][j] = model_normed_pgdelta;
      }
  glue_set_softenings();
}
