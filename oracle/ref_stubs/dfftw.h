/* Stand-in for FFTW-2's <dfftw.h>: see sfftw.h */
#include "sfftw.h"
