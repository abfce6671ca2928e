// grouped_report.hpp -- launchers of grouped_report_pass.hip, shared with capi_report_grouped.hpp (the grouped lin_reg_report)
#pragma once
#include "common.hpp"

namespace pds {

// Per-group t quantile and ln-gamma term of the epilogue, keyed by k = n_g - p' (the group's dof as an integer).  Both come from the
// host functions of stats.cpp (student_t_ppf(0.975, dof), student_t_lng_term(dof)), once per distinct dof: the CI stays
// bit-identical to the single report's.  k < dense_len: dense[2 k], dense[2 k + 1]; otherwise the sorted large_keys list.
struct ReportDofTable {
    int64_t dense_len = 0;
    const double* dense = nullptr;  // [dense_len][2]: t_alpha, lng
    int64_t n_large = 0;
    const int64_t* large_keys = nullptr;  // ascending
    const double* large = nullptr;        // [n_large][2]
};

// Second pass of the grouped report over a frame in group order: per group g of [d_off[g], d_off[g + 1]) (absolute rows)
//   d_sums[4 g + 0..2] = sum e^2, sum (y - y_first), sum (y - y_first)^2
//   hc > 0: d_meat[g] = X' diag(s) X as p' x p' column-major f64 (bias last), s = e^2 (hc 1), e^2 / (1 - h) (2), e^2 / (1 - h)^2 (3)
// Groups with fewer than p' rows are skipped (the epilogue nulls them).  d_cols: x_0 .. x_{p-1}, y.  1 .. 64 features.
// weighted (hc == 0 only): d_cols[p + 1] is the weight column and d_sums[4 g + 3] = sum w e^2 (0.0 otherwise), which the weighted
// epilogue's mse reads; sum e^2 and the y sums stay unweighted.
// Groups of more than piece_rows rows are split so that their rows stream on many waves: the first piece_rows rows stay the group's
// own item, the rest are the n_pieces extra items d_pieces[3 k ..] = (group, first row, end row) with their own sums / meat slots
// (d_sums / d_meat hold n_groups + n_pieces slots), folded back per group in piece order by d_fin[3 j ..] = (group, first extra
// item, count) -- deterministic: the same bits for every launch and every piece schedule.
template <typename T>
int launch_grouped_report_pass(pds_ctx* ctx, const T* const* d_cols, int n_feat, int bias, const int64_t* d_off, int64_t n_groups,
                               const T* d_beta, const T* d_inv, int hc, double* d_sums, double* d_meat, const int64_t* d_pieces,
                               int64_t n_pieces, int64_t piece_rows, const int64_t* d_fin, int64_t n_fin, bool weighted = false);

// report_epilogue (capi_report.hpp) per group, on the device: se, t, p, CI, r2, adj_r2 and the null flag.  d_beta is read and, for
// null groups, overwritten with NaN.  d_yvar (nullable): the caller's var(y) per group; null -> from d_sums (ddof = 1).
template <typename T>
int launch_grouped_report_epilogue(pds_ctx* ctx, const int64_t* d_off, int64_t n_groups, int n_feat, int bias, int se_type,
                                   const T* d_yvar, T* d_beta, const T* d_inv, const double* d_sums, const double* d_meat,
                                   const ReportDofTable& tab, T* se, T* t, T* p, T* lo, T* hi, T* r2, T* adj_r2, uint8_t* is_null,
                                   bool weighted = false);

// pass 1 of groups split into pieces: d_rec[g] = sum over k in [d_vfirst[g], d_vfirst[g + 1]) of d_vrec[k] ((p+2)^2 records, f64 sums)
template <typename T>
int launch_grouped_report_sum_records(pds_ctx* ctx, const T* d_vrec, const int64_t* d_vfirst, int64_t n_groups, int qq, T* d_rec);

// the device survival function on a grid (tests): out[i] = student_t_sf(x[i], df[i]) with lng[i] = student_t_lng_term(df[i])
int launch_student_t_sf_grid(pds_ctx* ctx, const double* d_x, const double* d_df, const double* d_lng, int64_t n, double* d_out);

}  // namespace pds
