// drgnn_step_tu.hip -- one translation unit of the fused step kernels' instantiations.
//   -DDRGNN_AF_FAM=AF_<family> -DDRGNN_AF_W=<16|32|48|64>: one (family, width) of the aggregation-first kernels (drgnn_step_af.h:
//       the unit instantiates that family's kernel lookup, which instantiates the kernels)
#include "drgnn_kernels.h"
#if !defined(DRGNN_AF_FAM) || !defined(DRGNN_AF_W)
#error "compile with -DDRGNN_AF_FAM=AF_<family> -DDRGNN_AF_W=<width>"
#endif
template const void* af_unit<DRGNN_AF_FAM, DRGNN_AF_W>(const AfKey&);
