// rescore_metric_f32.hip — the metric batched search's rescoring kernels for f32 rows (rescore.h):
// what the float32 filter (search_mfma_f32.hip) rescores with under dotproduct / euclidean.  A
// translation unit of its own, as the f16 and bf16 ones, so that they compile in parallel.
#include "rescore.h"

namespace rc {
template void launch_rescore_metric<float>(const BatchPlan &, const BatchWs &, int, hipStream_t);
}  // namespace rc
