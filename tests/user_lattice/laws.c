/* Host force laws and lattice corrections for tests/test_user_lattice.py, compiled with gcc into a shared library and handed
 * to the library as user-defined laws (ngravs_create_with_lattice).  The laws are copies of the reference's newtonian,
 * plummer, yukawa and coloyuk at addresses the library does not know; the lattice corrections are written from the Ewald and
 * screened-Ewald sums the library's own tables use, in box units (x = 0.5 (i, j, k) / 64), and a plain image sum for a
 * screened law that has no built-in counterpart. */
#include <math.h>

static double Box = 1.0;          /* BoxSize of the run: the laws' length scales are fixed in units of the box */
static double YukawaImass = 60.0; /* YUKAWA_IMASS: Yukawa mass times the box */
static double ScreenLen = 0.1;    /* screened law: screening length in units of the box */

void fx_set_box(double box) { Box = box; }
void fx_set_yukawa_imass(double m) { YukawaImass = m; }
void fx_set_screen_len(double l) { ScreenLen = l; }

double fx_newton(double t, double s, double r2, double r, long n)
{
  (void)t; (void)r; (void)n;
  return s / r2;
}

double fx_plummer(double t, double s, double h, double r, long n)
{
  double hi = 1.0 / h, u = r * hi;
  (void)t; (void)n;
  if(u < 0.5)
    return s * hi * hi * hi * (10.666666666667 + u * u * (32.0 * u - 38.4));
  return s * hi * hi * hi * (21.333333333333 - 48.0 * u + 38.4 * u * u - 10.666666666667 * u * u * u - 0.066666666667 / (u * u * u));
}

double fx_yukawa(double t, double s, double r2, double r, long n)
{
  double ym = YukawaImass / Box;
  (void)t; (void)n;
  return s * exp(-r * ym) * (ym / r + 1.0 / r2);
}

double fx_coloyuk(double t, double s, double r2, double r, long n) { return fx_yukawa(t, s, r2, r, n) + s / r2; }

/* screened law, no built-in counterpart: F = m exp(-r / (ScreenLen Box)) / r^2 */
double fx_screened(double t, double s, double r2, double r, long n)
{
  (void)t; (void)n;
  return s * exp(-r / (ScreenLen * Box)) / r2;
}

/* Ewald sum of the 1/r^2 force minus the nearest image (alpha = 2, 9^3 real and reciprocal vectors) */
void fx_ewald_lattice(int i, int j, int k, double x[3], double force[3])
{
  const double alpha = 2.0;
  double r2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2], g[3];
  int a, b, c, d;

  if(i == 0 && j == 0 && k == 0)
    return;
  for(d = 0; d < 3; d++)
    g[d] = x[d] / (r2 * sqrt(r2));
  for(a = -4; a <= 4; a++)
    for(b = -4; b <= 4; b++)
      for(c = -4; c <= 4; c++)
        {
          double dx[3] = {x[0] - a, x[1] - b, x[2] - c};
          double r = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
          double w = erfc(alpha * r) + 2 * alpha * r / sqrt(M_PI) * exp(-alpha * alpha * r * r);
          for(d = 0; d < 3; d++)
            g[d] -= dx[d] / (r * r * r) * w;
        }
  for(a = -4; a <= 4; a++)
    for(b = -4; b <= 4; b++)
      for(c = -4; c <= 4; c++)
        {
          int h2 = a * a + b * b + c * c;
          if(h2 > 0)
            {
              double w = 2.0 / h2 * exp(-M_PI * M_PI * h2 / (alpha * alpha)) * sin(2 * M_PI * (x[0] * a + x[1] * b + x[2] * c));
              g[0] -= a * w;
              g[1] -= b * w;
              g[2] -= c * w;
            }
        }
  for(d = 0; d < 3; d++)
    force[d] += g[d];
}

/* screened Ewald sum of the Yukawa force minus the nearest image (alpha = 5.64, 11^3 vectors); like the reference's
 * yukawa_lattice_force it returns at the origin without writing force[] */
void fx_yukawa_lattice(int i, int j, int k, double x[3], double force[3])
{
  const double alpha = 5.64;
  double ym = YukawaImass, r2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2], r = sqrt(r2), g[3];
  int a, b, c, d;

  if(i == 0 && j == 0 && k == 0)
    return;
  for(d = 0; d < 3; d++)
    g[d] = exp(-r * ym) * (ym + 1.0 / r) * x[d] / r2;
  for(a = -5; a <= 5; a++)
    for(b = -5; b <= 5; b++)
      for(c = -5; c <= 5; c++)
        {
          double dx[3] = {x[0] - a, x[1] - b, x[2] - c};
          double q = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
          double ep = exp(ym * q) * erfc(alpha * q + ym / (2 * alpha)), em = exp(-ym * q) * erfc(alpha * q - ym / (2 * alpha));
          double w1 = 0.5 * (ep + em);
          double w2 = 0.5 * ym * (-ep + em) + 2 * alpha * exp(-alpha * alpha * q * q - ym * ym / (4 * alpha * alpha)) / sqrt(M_PI);
          for(d = 0; d < 3; d++)
            g[d] -= dx[d] / (q * q * q) * w1;
          for(d = 0; d < 3; d++)
            g[d] -= dx[d] / (q * q) * w2;
        }
  ym /= 2 * M_PI;
  for(a = -5; a <= 5; a++)
    for(b = -5; b <= 5; b++)
      for(c = -5; c <= 5; c++)
        {
          int h2 = a * a + b * b + c * c;
          if(h2 > 0)
            {
              double w = 2 * exp(-M_PI * M_PI * (h2 + ym * ym) / (alpha * alpha)) * sin(2 * M_PI * (x[0] * a + x[1] * b + x[2] * c)) /
                         (h2 + ym * ym);
              g[0] -= a * w;
              g[1] -= b * w;
              g[2] -= c * w;
            }
        }
  for(d = 0; d < 3; d++)
    force[d] += g[d];
}

void fx_coloyuk_lattice(int i, int j, int k, double x[3], double force[3])
{
  fx_ewald_lattice(i, j, k, x, force);
  fx_yukawa_lattice(i, j, k, x, force);
}

/* the screened law's images: -sum over n != 0, |n_i| <= 3, of F(|x - n|) (x - n) / |x - n| in box units (the terms beyond fall
 * below exp(-2.5 / ScreenLen)) */
void fx_screened_lattice(int i, int j, int k, double x[3], double force[3])
{
  int a, b, c, d;

  (void)i; (void)j; (void)k;
  for(a = -3; a <= 3; a++)
    for(b = -3; b <= 3; b++)
      for(c = -3; c <= 3; c++)
        if(a || b || c)
          {
            double dx[3] = {x[0] - a, x[1] - b, x[2] - c};
            double r = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
            double f = exp(-r / ScreenLen) / (r * r * r);
            for(d = 0; d < 3; d++)
              force[d] -= f * dx[d];
          }
}

/* a lattice function that goes wrong at one point */
void fx_nan_lattice(int i, int j, int k, double x[3], double force[3])
{
  (void)x;
  if(i == 3 && j == 4 && k == 5)
    force[1] = NAN;
}
