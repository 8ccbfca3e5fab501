// nsd_multi_window48.hip -- the model-batched twin of nsd_window48.hip (nsd_multi.h): nsd_multi_window_step's kernel, its mean kernel
// and their launcher, in a translation unit of their own so that the single-model kernels are compiled exactly as before.
#define NSD_MULTI_TU 1
#include "nsd_window48.hip"
