// Host-side dispatch of a runtime value to a compile-time template argument.
//
// A launcher nests these and writes its hipLaunchKernelGGL once, inside the
// innermost generic lambda; each level hands its choice down as a
// std::integral_constant, read back with decltype(x)::value. The lists of
// values given here ARE the instantiation set of a kernel.
#pragma once

#include <torch/extension.h>

#include <type_traits>

template <int N>
using Int = std::integral_constant<int, N>;

// f(Int<N>{}) for the N in Ns equal to `value`; an error naming `what` when
// there is none.
template <int... Ns, typename F>
void dispatch_int(const int value, const char* what, F&& f) {
  const bool hit = ((value == Ns ? (f(Int<Ns>{}), true) : false) || ...);
  TORCH_CHECK(hit, "unsupported ", what, " ", value);
}

template <typename F>
void dispatch_bool(const bool flag, F&& f) {
  if (flag)
    f(std::true_type{});
  else
    f(std::false_type{});
}
