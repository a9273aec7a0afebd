// deep_scores_f32.hip — instantiates the deep top-k score pass (contiguous and page-table, every metric) for f32 rows.
#include "deep_scores.h"

namespace rc {
template void launch_deep_scores<float>(const DeepScoreArgs &a);
}  // namespace rc
