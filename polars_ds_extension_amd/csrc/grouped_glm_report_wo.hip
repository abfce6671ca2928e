// grouped_glm_report_wo.hip -- the WO = true instantiations (a prior weight and an offset per row) of the report, piece and fold
// kernel templates of grouped_glm_report.hip, in a translation unit of their own so that the two sets of 96 kernels compile side by
// side.  The code is grouped_glm_report.hip's; the launchers of common.hpp, which live there, reach these through
// GroupedGlmReportSet<T, true>.
#define PDS_GLM_REPORT_WO 1
#include "grouped_glm_report.hip"
