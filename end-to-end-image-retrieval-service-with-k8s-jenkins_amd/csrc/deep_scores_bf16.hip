// deep_scores_bf16.hip — instantiates the deep top-k score pass (contiguous and page-table, every metric) for bf16 rows.
#include "deep_scores.h"

namespace rc {
template void launch_deep_scores<bf16_t>(const DeepScoreArgs &a);
}  // namespace rc
