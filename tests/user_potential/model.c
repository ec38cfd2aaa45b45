/* A test model's potential companions for ngravs_create_with_potentials: what a model author would put next to the force laws
 * in the model's own wiring.  The functions have the reference's `gravity` and `latpot` signatures.  The tests hold the library
 * to what these functions say, not to physics: the Yukawa spline companion is deliberately no multiple of the Plummer one. */
#include <math.h>

static double mdl_mu = 0.0;    /* inverse screening length, per unit length */
static double mdl_box = 1.0;   /* box size: the lattice functions work in box units */
void mdl_set(double mu, double box)
{
  mdl_mu = mu;
  mdl_box = box;
}

#define UNUSED(a, b, c) ((void)(a), (void)(b), (void)(c))

/* ---- Newton and Plummer: +source / r, and the spline potential of the softened point mass ---- */
double mdl_newton_pot(double t, double s, double h, double r, long N)
{
  UNUSED(t, h, N);
  return s / r;
}
double mdl_neg_newton_pot(double t, double s, double h, double r, long N) { return -mdl_newton_pot(t, s, h, r, N); }
double mdl_plummer_pot(double t, double s, double h, double r, long N)
{
  const double h_inv = 1 / h;
  UNUSED(t, N, 0);
  r *= h_inv;
  if(r < 0.5)
    return s * h_inv * (-2.8 + r * r * (5.333333333333 + r * r * (6.4 * r - 9.6)));
  return s * h_inv * (-3.2 + 0.066666666667 / r + r * r * (10.666666666667 + r * (-16.0 + r * (9.6 - 2.133333333333 * r))));
}
double mdl_neg_plummer_pot(double t, double s, double h, double r, long N) { return -mdl_plummer_pot(t, s, h, r, N); }

/* ---- Yukawa: s exp(-mu r) / r, and a smooth spline companion of its own ---- */
double mdl_yuk_pot(double t, double s, double h, double r, long N)
{
  UNUSED(t, h, N);
  return s * exp(-mdl_mu * r) / r;
}
double mdl_yuk_spline(double t, double s, double h, double r, long N)
{
  const double u = r / h;
  UNUSED(t, N, 0);
  return -s / h * (2.8 - 1.7 * u * u + 0.4 * u * u * u * u * u) * exp(-mdl_mu * r);
}
/* Newton + Yukawa, the companions of the coloyuk force law */
double mdl_coloyuk_pot(double t, double s, double h, double r, long N) { return mdl_newton_pot(t, s, h, r, N) + mdl_yuk_pot(t, s, h, r, N); }
double mdl_coloyuk_spline(double t, double s, double h, double r, long N)
{
  return mdl_plummer_pot(t, s, h, r, N) + mdl_yuk_spline(t, s, h, r, N);
}

/* ---- lattice potentials, x in box units in one octant ---- */
/* the periodic images of the Yukawa potential as a plain sum: images beyond |n_i| <= 6 are below exp(-33) at mu box = 6 */
double mdl_yuk_psi(double x[3])
{
  const double mu = mdl_mu * mdl_box;
  const double r0 = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  double sum = 0;
  int n0, n1, n2;
  for(n0 = -6; n0 <= 6; n0++)
    for(n1 = -6; n1 <= 6; n1++)
      for(n2 = -6; n2 <= 6; n2++)
        {
          const double d0 = x[0] - n0, d1 = x[1] - n1, d2 = x[2] - n2;
          const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
          sum += exp(-mu * r) / r;
        }
  return exp(-mu * r0) / r0 - sum;
}
/* Ewald's sum for the Newtonian lattice potential, alpha = 2, images and wave vectors to |n_i|, |h_i| <= 4 */
double mdl_ewald_psi(double x[3])
{
  const double alpha = 2.0, pi = 3.14159265358979323846;
  const double r0 = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  double sum1 = 0, sum2 = 0;
  int a, b, c;
  for(a = -4; a <= 4; a++)
    for(b = -4; b <= 4; b++)
      for(c = -4; c <= 4; c++)
        {
          const double d0 = x[0] - a, d1 = x[1] - b, d2 = x[2] - c;
          const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
          sum1 += erfc(alpha * r) / r;
        }
  for(a = -4; a <= 4; a++)
    for(b = -4; b <= 4; b++)
      for(c = -4; c <= 4; c++)
        {
          const int h2 = a * a + b * b + c * c;
          if(h2 > 0)
            sum2 += 1 / (pi * h2) * exp(-pi * pi * h2 / (alpha * alpha)) * cos(2 * pi * (x[0] * a + x[1] * b + x[2] * c));
        }
  return pi / (alpha * alpha) - sum1 - sum2 + 1 / r0;
}
double mdl_other_psi(double x[3]) { return 2 * mdl_ewald_psi(x); }
double mdl_nan_psi(double x[3]) { return x[0] == 3 * 0.5 / 64 && x[1] == 4 * 0.5 / 64 && x[2] == 5 * 0.5 / 64 ? NAN : 1.0; }

/* ---- what ngravs_create_with_potentials refuses ---- */
double mdl_twice_pot(double t, double s, double h, double r, long N) { return 2 * mdl_newton_pot(t, s, h, r, N); }          /* third law */
double mdl_twice_spline(double t, double s, double h, double r, long N) { return 2 * mdl_plummer_pot(t, s, h, r, N); }
double mdl_quadratic_pot(double t, double s, double h, double r, long N) { return s * mdl_newton_pot(t, s, h, r, N); }      /* source^2 */
double mdl_target_pot(double t, double s, double h, double r, long N) { return t * mdl_newton_pot(t, s, h, r, N); }
double mdl_count_pot(double t, double s, double h, double r, long N) { return (double)N * mdl_newton_pot(t, s, h, r, N); }
double mdl_count_spline(double t, double s, double h, double r, long N) { return (double)N * mdl_plummer_pot(t, s, h, r, N); }
double mdl_soft_pot(double t, double s, double h, double r, long N)
{
  UNUSED(t, N, 0);
  return s / sqrt(r * r + h * h);                                                                                            /* depends on h */
}
