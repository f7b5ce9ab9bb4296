// ks_panel.h -- what the analyses of row-normalised spectra share (ks_pca,
// ks_kmeans, ks_kmeans_seed, ks_knn; the checks and the upload also
// ks_spectra_dist): the row-major FP64 profile panel and the checks of its
// rows, on the device and on the host, the checks of the arguments that
// describe a selection, and the uploads of a host-buffer entry point.
// DESIGN.md 6p.
#pragma once
#include "ks_internal.h"

namespace ks {

// The checks of a selection's arguments, each with the entry point's own limit
// and wording; an entry point calls them in its own order.
// "<what> needs at least <least> <unit>[s] (<name> = <m>)"
ks_status panel_check_count(int64_t m, int64_t least, const char *what, const char *unit, const char *name);
ks_status panel_check_most(int64_t m, int64_t most);
ks_status panel_check_ncol(int32_t ncol, int32_t most);
ks_status panel_check_n(int64_t n);
// A NULL selection of cnt rows is rows 0 .. cnt - 1.
ks_status panel_check_null_rows(const void *rows, int64_t cnt, int64_t n, const char *rows_name, const char *cnt_name);
// The checks k-means, group means and seeding share: m >= 1, ncol <= KS_DIST_MAX_NCOL, no flags.
ks_status panel_check_common(int64_t n, int32_t ncol, const void *rows, int64_t m, int32_t flags, const char *what);

// The metric field of distance flags whose other bits the caller has checked:
// "unknown distance metric N" above KS_DIST_HELLINGER, and KS_DIST_SQUARED is
// refused with a metric that has no squared form.
ks_status dist_check_metric(int32_t flags);

// What a panel entry is: the profile p, or its root (the Hellinger panel).
enum class PanelRoot { kNone, kSqrt };

// Queues k_panel_normalise on ctx->stream for one selection (rows null: rows
// 0 .. cnt - 1): panel[s][c] = count / row sum, row-major [cnt][ncol]; with
// PanelRoot::kSqrt the correctly rounded root of that.  iota
// (may be null): iota[s] = s.  bad_index / bad_empty (device words the caller
// zeroed): cnt - s of the first bad row index / of the first row without
// counts, by atomicMax.  No synchronisation: the caller reads the words back.
ks_status panel_normalise(ks_ctx *ctx, const uint32_t *sp, int64_t n, int ncol, const int64_t *rows, int64_t cnt,
                          PanelRoot root, double *panel, int *iota, unsigned long long *bad_index,
                          unsigned long long *bad_empty);
// The words read back, for one or two selections (sides): bad[0 .. sides) are
// the bad_index words, bad[sides .. 2 sides) the bad_empty words.  The first
// selection's index comes first, then the second's, then the empty rows.
ks_status panel_report(const unsigned long long *bad, int sides, int64_t na, int64_t nb);
// The host forms of the same checks, reported as the device reports them: the
// indices of one selection (side 0 or 1; rows null: nothing to check) ...
ks_status panel_check_index_host(const int64_t *rows, int64_t cnt, int64_t n, int side);
// ... and, for one selection (rows_b null) or two, all indices, then all row sums.
ks_status panel_check_rows_host(const uint32_t *spectra, int64_t n, int ncol, const int64_t *rows, int64_t na,
                                const int64_t *rows_b, int64_t nb);

// The uploads of a host-buffer entry point: the spectra into SLOT_COUNTS, up
// to two selections behind one another in SLOT_REGIONS (null for a NULL
// selection; nb rows are kept for the second one either way), then `extra`
// int64 the caller fills or reads.  Asynchronous, on ctx->stream.
struct SpectraUpload {
  const uint32_t *sp = nullptr;
  int64_t *rows = nullptr, *rows_b = nullptr, *extra = nullptr;
};
ks_status upload_spectra(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int ncol, const int64_t *rows, int64_t na,
                         const int64_t *rows_b, int64_t nb, int64_t extra, SpectraUpload *up);

}  // namespace ks
