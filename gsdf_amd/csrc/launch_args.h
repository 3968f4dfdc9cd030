// launch_args.h -- the marshalling step of a kernel launch, host only (no HIP include: tests/test_launch_args.py compiles it with
// g++). The arguments of a call are converted to the kernel's own parameter types P... into storage of their own, and args[i]
// points at parameter i: the array hipModuleLaunchKernel takes (abi_program.h: launch_kernel).
#pragma once
#include <cstddef>
#include <tuple>
#include <type_traits>
#include <utility>

namespace launch_args {

template <typename P, typename A, typename = void>
struct castable : std::false_type {};
template <typename P, typename A>
struct castable<P, A, std::void_t<decltype(static_cast<P>(std::declval<A>()))>> : std::true_type {};

template <bool SameCount, typename Params, typename... A>
struct all_castable : std::false_type {};
template <typename... P, typename... A>
struct all_castable<true, std::tuple<P...>, A...> : std::bool_constant<(castable<P, A>::value && ...)> {};

// accepts<void(P...), A...>: as many arguments as parameters, each convertible by static_cast
template <typename Sig, typename... A>
struct accepts : std::false_type {};
template <typename... P, typename... A>
struct accepts<void(P...), A...> : all_castable<sizeof...(P) == sizeof...(A), std::tuple<P...>, A...> {};

template <typename Sig>
class Marshalled;
template <typename... P>
class Marshalled<void(P...)> {
 public:
  static constexpr size_t N = sizeof...(P);
  template <typename... A>
  explicit Marshalled(const A&... a) : v_(static_cast<P>(a)...) {
    static_assert(accepts<void(P...), const A&...>::value, "kernel launch: argument count or types do not fit the kernel's signature");
    fill(std::index_sequence_for<P...>{});
  }
  Marshalled(const Marshalled&) = delete;
  Marshalled& operator=(const Marshalled&) = delete;
  void** args() { return args_; }
 private:
  template <size_t... I>
  void fill(std::index_sequence<I...>) { ((args_[I] = (void*)&std::get<I>(v_)), ...); }
  std::tuple<std::remove_cv_t<P>...> v_;
  void* args_[N ? N : 1] = {};
};

}  // namespace launch_args
