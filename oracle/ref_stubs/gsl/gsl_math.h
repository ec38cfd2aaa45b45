/* Stand-in for <gsl/gsl_math.h>: the two macros the reference's headers expect to exist. */
#ifndef NGRAVS_REF_STUB_GSL_MATH_H
#define NGRAVS_REF_STUB_GSL_MATH_H
#define GSL_MAX(a, b) ((a) > (b) ? (a) : (b))
#define GSL_MIN(a, b) ((a) < (b) ? (a) : (b))
#endif
