// knn_grid_d3.hip -- instantiates the grid search kernels (knn_grid_search.h) for D = 3.
#include "knn_grid_search.h"
#include "knn_grid_box.h"

namespace pointops {

template void grid_search<3, kRunBitsStd>(const KnnArgs&, const GridWs&, int, int, bool);

}  // namespace pointops
