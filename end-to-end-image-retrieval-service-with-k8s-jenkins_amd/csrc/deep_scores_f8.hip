// deep_scores_f8.hip — instantiates the deep top-k score pass (contiguous and page-table, every metric) for float8 rows.
#include "deep_scores.h"

namespace rc {
template void launch_deep_scores<f8_t>(const DeepScoreArgs &a);
}  // namespace rc
