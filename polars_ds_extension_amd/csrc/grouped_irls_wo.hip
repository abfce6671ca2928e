// grouped_irls_wo.hip -- the weighted / offset kernels (PEN = 3: a prior weight and an offset per row, unpenalised) of
// grouped_irls.hip and their launcher, in a translation unit of their own so that the four sets of 32 kernels compile side by side.
// The code is grouped_irls.hip's.
#define PDS_GROUPED_IRLS_PEN 3
#include "grouped_irls.hip"
