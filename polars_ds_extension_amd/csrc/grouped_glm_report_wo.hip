// grouped_glm_report_wo.hip -- the weighted / offset kernels (a prior weight and an offset per row) of grouped_glm_report.hip and
// their launchers, in a translation unit of their own: the kernels of grouped_glm_report.hip keep their objects.
// The code is grouped_glm_report.hip's.
#define PDS_GLM_REPORT_WO 1
#include "grouped_glm_report.hip"
