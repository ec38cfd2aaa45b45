/* A model's own ngravs.c in miniature, with its lattice corrections: copies of newtonian / coloyuk / plummer at addresses the
 * glue does not know, and the LatticeForce[l][m] array the reference's allvars.h declares, holding the model's own Ewald and
 * screened-Ewald corrections for those copies.  Linked into tests/glue_stub/glue_driver.c with gadget_glue.c built with
 * -Dset_softenings=glue_set_softenings: the driver's set_softenings() call (init.c:60) lands here, re-wires the driver's
 * built-in Newton / Coloyuk / Plummer slots to the copies, fills LatticeForce, and goes on into the glue's own set_softenings.
 * The Green's functions stay the built-in ones. */
#include <math.h>
#include "allvars.h"
#include "proto.h"
#include "ngravs.h"

typedef void (*latforce)(int, int, int, double *, double *);   /* allvars.h:138 of the reference */
latforce LatticeForce[N_GRAVS][N_GRAVS];

void glue_set_softenings(void);

static double model_newtonian(double target, double source, double h, double r, long N)
{
  (void)target;
  (void)r;
  (void)N;
  return source / h;
}
static double model_coloyuk(double target, double source, double h, double r, long N)
{
  double ym = YUKAWA_IMASS / All.BoxSize;

  (void)target;
  (void)N;
  return source * exp(-r * ym) * (ym / r + 1.0 / h) + source / h;
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

/* Ewald sum of the 1/r^2 force minus the nearest image, box units */
static void model_ewald(int i, int j, int k, double *x, double *force)
{
  const double alpha = 2.0;
  double r2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  int a, b, c, d;

  if(i == 0 && j == 0 && k == 0)
    return;
  for(d = 0; d < 3; d++)
    force[d] += x[d] / (r2 * sqrt(r2));
  for(a = -4; a <= 4; a++)
    for(b = -4; b <= 4; b++)
      for(c = -4; c <= 4; c++)
        {
          double dx[3] = {x[0] - a, x[1] - b, x[2] - c};
          double r = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
          double w = erfc(alpha * r) + 2 * alpha * r / sqrt(M_PI) * exp(-alpha * alpha * r * r);
          int h2 = a * a + b * b + c * c;

          for(d = 0; d < 3; d++)
            force[d] -= dx[d] / (r * r * r) * w;
          if(h2 > 0)
            {
              double v = 2.0 / h2 * exp(-M_PI * M_PI * h2 / (alpha * alpha)) * sin(2 * M_PI * (x[0] * a + x[1] * b + x[2] * c));
              force[0] -= a * v;
              force[1] -= b * v;
              force[2] -= c * v;
            }
        }
}

/* screened Ewald sum of the Yukawa force minus the nearest image (ym = YUKAWA_IMASS in box units) */
static void model_yukawa_lattice(int i, int j, int k, double *x, double *force)
{
  const double alpha = 5.64;
  double ym = YUKAWA_IMASS, r2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2], r = sqrt(r2), yk;
  int a, b, c, d;

  if(i == 0 && j == 0 && k == 0)
    return;
  for(d = 0; d < 3; d++)
    force[d] += exp(-r * ym) * (ym + 1.0 / r) * x[d] / r2;
  yk = ym / (2 * M_PI);
  for(a = -5; a <= 5; a++)
    for(b = -5; b <= 5; b++)
      for(c = -5; c <= 5; c++)
        {
          double dx[3] = {x[0] - a, x[1] - b, x[2] - c};
          double q = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
          double ep = exp(ym * q) * erfc(alpha * q + ym / (2 * alpha)), em = exp(-ym * q) * erfc(alpha * q - ym / (2 * alpha));
          double w1 = 0.5 * (ep + em);
          double w2 = 0.5 * ym * (-ep + em) + 2 * alpha * exp(-alpha * alpha * q * q - ym * ym / (4 * alpha * alpha)) / sqrt(M_PI);
          int h2 = a * a + b * b + c * c;

          for(d = 0; d < 3; d++)
            force[d] -= dx[d] / (q * q * q) * w1;
          for(d = 0; d < 3; d++)
            force[d] -= dx[d] / (q * q) * w2;
          if(h2 > 0)
            {
              double v = 2 * exp(-M_PI * M_PI * (h2 + yk * yk) / (alpha * alpha)) * sin(2 * M_PI * (x[0] * a + x[1] * b + x[2] * c)) /
                         (h2 + yk * yk);
              force[0] -= a * v;
              force[1] -= b * v;
              force[2] -= c * v;
            }
        }
}
static void model_coloyuk_lattice(int i, int j, int k, double *x, double *force)
{
  model_ewald(i, j, k, x, force);
  model_yukawa_lattice(i, j, k, x, force);
}

void set_softenings(void)
{
  int i, j;

  for(i = 0; i < N_GRAVS; i++)
    for(j = 0; j < N_GRAVS; j++)
      {
        LatticeForce[i][j] = 0;
        if(AccelFxns[i][j] == newtonian)
          {
            AccelFxns[i][j] = model_newtonian;
            LatticeForce[i][j] = model_ewald;
          }
        else if(AccelFxns[i][j] == coloyuk)
          {
            AccelFxns[i][j] = model_coloyuk;
            LatticeForce[i][j] = model_coloyuk_lattice;
          }
        if(AccelSplines[i][j] == plummer)
          AccelSplines[i][j] = model_plummer;
      }
  glue_set_softenings();
}
