/* Stand-in for R's R.h: what the reference solver's two translation units need from it. */
#include <stdio.h>
#include <stdlib.h>
#include <limits.h>
#include <math.h>
#include <string.h>
#define Rprintf printf
