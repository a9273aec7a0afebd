// deep_scores_f16.hip — instantiates the deep top-k score pass (contiguous and page-table, every metric) for f16 rows.
#include "deep_scores.h"

namespace rc {
template void launch_deep_scores<f16_t>(const DeepScoreArgs &a);
}  // namespace rc
