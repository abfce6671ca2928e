// grouped_irls_ridge.hip -- the ridge kernels (PEN = 1: n l2 on the feature diagonal of every IRLS step) of
// grouped_irls.hip and their launcher, in a translation unit of their own so that the three sets of 32 kernels compile side by side.
// The code is grouped_irls.hip's.
#define PDS_GROUPED_IRLS_PEN 1
#include "grouped_irls.hip"
