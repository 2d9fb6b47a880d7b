// A kernel form chosen at run time, its launch written once: f gets the template argument as an
// std::integral_constant (f(std::true_type{}) / f(std::false_type{}); the grid's dimension 2 / 3;
// the waves per file 4 / 2 / 1 of K1's file-ordered count pass).  Shared by the host drivers of
// stdbscan.hip and polar.hip.  A site where one of the forms must not be instantiated keeps a
// plain `if`.
#pragma once
#include <type_traits>

namespace rpt {

template <class F>
auto with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
template <class F>
auto with_dim(int dim, F&& f) {
  return dim == 2 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 3>{});
}
// w is 4 or 2, anything else takes the one-wave form
template <class F>
auto with_waves(int w, F&& f) {
  return w == 4   ? f(std::integral_constant<int, 4>{})
         : w == 2 ? f(std::integral_constant<int, 2>{})
                  : f(std::integral_constant<int, 1>{});
}

}  // namespace rpt
