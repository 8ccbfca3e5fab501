// nsd_lstm2_multi_fwd48x4.hip -- the model-batched twin of nsd_lstm2_fwd48x4.hip (nsd_multi.h): its multi-model kernel and launcher, in a
// translation unit of their own so that the single-model kernels are compiled exactly as before.
#define NSD_MULTI_TU 1
#include "nsd_lstm2_fwd48x4.hip"
