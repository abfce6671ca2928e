// grouped_irls_cd.hip -- the coordinate-descent kernels (PEN = 2: the elastic-net IRLS step, l1_reg > 0) of
// grouped_irls.hip and their launcher, in a translation unit of their own so that the three sets of 32 kernels compile side by side.
// The code is grouped_irls.hip's.
#define PDS_GROUPED_IRLS_PEN 2
#include "grouped_irls.hip"
