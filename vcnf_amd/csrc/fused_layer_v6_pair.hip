// Fused RQS coupling layers, fp16 split-half matrix path: TWO layers per tile visit at large batches
// (fused_rqs_layer_v6_pair_kernel).  The kernel is the body of fused_layer_v6.hip with its layer loop of two trips and
// two table sets in LDS (LdsV6Pair); everything that differs is under VCNF_V6_PAIR there.  A unit of its own, one per
// number of residual blocks (-DVCNF_V6_NBLK=1|2|3), so that the one-layer units compile exactly what they did.
#define VCNF_V6_PAIR 1
#include "fused_layer_v6.hip"
