/* oracle/ref_shim: the reference includes the profiler API and calls none of it. */
#include "cuda_runtime.h"
