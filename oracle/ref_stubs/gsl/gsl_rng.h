/* Stand-in for <gsl/gsl_rng.h>: the reference only holds a pointer to a generator on the SPH path; drawing from it is a
 * harness error (ref_stubs.c aborts). */
#ifndef NGRAVS_REF_STUB_GSL_RNG_H
#define NGRAVS_REF_STUB_GSL_RNG_H
typedef struct ngravs_ref_stub_rng gsl_rng;
double gsl_rng_uniform(const gsl_rng *r);
#endif
