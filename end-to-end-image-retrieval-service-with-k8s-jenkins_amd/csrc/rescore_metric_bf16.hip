// rescore_metric_bf16.hip — the metric batched search's rescoring kernels for bf16 rows (rescore.h):
// one of two per-dtype translation units, so that they compile in parallel.
#include "rescore.h"

namespace rc {
template void launch_rescore_metric<bf16_t>(const BatchPlan &, const BatchWs &, int, hipStream_t);
}  // namespace rc
