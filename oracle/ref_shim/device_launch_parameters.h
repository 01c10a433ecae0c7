/* oracle/ref_shim: threadIdx, blockIdx, blockDim and gridDim live in cuda_runtime.h. */
#include "cuda_runtime.h"
