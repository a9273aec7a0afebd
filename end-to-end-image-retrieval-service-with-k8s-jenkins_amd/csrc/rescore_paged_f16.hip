// rescore_paged_f16.hip — the paged batched search's rescoring kernels for f16 pool rows (rescore.h),
// cosine and metric: one of two per-dtype translation units, so that they compile in parallel.
#include "rescore.h"

namespace rc {
template void launch_rescore_paged<f16_t>(const BatchPlan &, const BatchWs &, int, hipStream_t);
}  // namespace rc
