// knn_grid_d3w.hip -- instantiates the grid search kernels (knn_grid_search.h) for D = 3, clouds of more than 2^21 - 16 points
// (8-bit run lengths: knn_grid_search.h, kRunBitsBig).
#include "knn_grid_search.h"
#include "knn_grid_box.h"

namespace pointops {

template void grid_search<3, kRunBitsBig>(const KnnArgs&, const GridWs&, int, int, bool);

}  // namespace pointops
