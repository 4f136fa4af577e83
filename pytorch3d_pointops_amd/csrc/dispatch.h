// dispatch.h -- host-only mapping of runtime values to template instances.  Each helper calls a generic lambda with
// std::integral_constant<int, V> for the chosen V and returns what it returns:
//   with_bucket(Ints<1, 2, 4>{}, K, f)      the smallest listed V >= v (list ascending), else the last one
//   with_exact<0>(Ints<2, 3>{}, D, f)       the listed V == v, else the fallback named at the call
// Value lists that several launch sites must agree on are named once (kScanKC, kGridKC, kFpsPpt).
#pragma once
#include <type_traits>

namespace pointops {

template <int... Vs>
struct Ints {};

template <int V>
using IntC = std::integral_constant<int, V>;

template <int V, int... Vs, class F>
auto with_bucket(Ints<V, Vs...>, int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) {
    return f(IntC<V>{});
  } else {
    if (v <= V) return f(IntC<V>{});
    return with_bucket(Ints<Vs...>{}, v, f);
  }
}

template <int Fallback, class F>
auto with_exact(Ints<>, int, F&& f) {
  return f(IntC<Fallback>{});
}

template <int Fallback, int V, int... Vs, class F>
auto with_exact(Ints<V, Vs...>, int v, F&& f) {
  if (v == V) return f(IntC<V>{});
  return with_exact<Fallback>(Ints<Vs...>{}, v, f);
}

}  // namespace pointops
