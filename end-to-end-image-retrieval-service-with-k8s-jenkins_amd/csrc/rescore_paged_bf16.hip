// rescore_paged_bf16.hip — the paged batched search's rescoring kernels for bf16 pool rows (rescore.h),
// cosine and metric: one of two per-dtype translation units, so that they compile in parallel.
#include "rescore.h"

namespace rc {
template void launch_rescore_paged<bf16_t>(const BatchPlan &, const BatchWs &, int, hipStream_t);
}  // namespace rc
