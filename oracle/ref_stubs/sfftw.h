/* Stand-in for FFTW-2's <sfftw.h>: one opaque handle type; no FFT is planned or run on the SPH path. */
#ifndef NGRAVS_REF_STUB_FFTW_H
#define NGRAVS_REF_STUB_FFTW_H
typedef void *fftw_plan;
#endif
