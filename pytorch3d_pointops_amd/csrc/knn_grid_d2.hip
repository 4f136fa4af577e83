// knn_grid_d2.hip -- instantiates the grid search kernels (knn_grid_search.h) for D = 2.
#include "knn_grid_search.h"
#include "knn_grid_box.h"

namespace pointops {

template void grid_search<2, kRunBitsStd>(const KnnArgs&, const GridWs&, int, int, bool);

}  // namespace pointops
