// A kernel instantiation and its profiling label from ONE spelling of its template arguments (host side).
// The label is the demangled name as nm -C and rocprof print it: the name as written, then the argument
// VALUES separated by ", ", bools as true / false -- so a PIPNET_KREF site writes every defaulted argument out.
#pragma once
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "../../include/pipnet_amd.h"

namespace pipnet {

struct TArg {                 // one int or bool template argument
  int v;
  bool is_bool;
  TArg(int x) : v(x), is_bool(false) {}
  TArg(bool x) : v(x), is_bool(true) {}
};
// "name<first, args...>" (first: an already formatted leading type argument, or empty); one shared copy
__attribute__((noinline)) inline std::string kernel_label(const char* name, std::initializer_list<TArg> args,
                                                          const std::string& first = "") {
  std::string s = std::string(name) + "<" + first;
  for (const TArg& a : args)
    s += (s.back() == '<' ? "" : ", ") + (a.is_bool ? std::string(a.v ? "true" : "false") : std::to_string(a.v));
  return s + ">";
}

template <class... Args>
struct KernelRef {
  void (*fn)(Args...) = nullptr;      // nullptr: no instantiation for what was asked
  std::string (*label)() = nullptr;   // formatted on request only: a launch never pays for it
};
// KernelRef of NAME<args...>; PIPNET_KREF_T takes a leading type argument that has a static label().
#define PIPNET_KREF(NAME, ...) \
  { &NAME<__VA_ARGS__>, [] { return pipnet::kernel_label(#NAME, {__VA_ARGS__}); } }
#define PIPNET_KREF_T(NAME, T, ...) \
  { &NAME<T, __VA_ARGS__>, [] { return pipnet::kernel_label(#NAME, {__VA_ARGS__}, T::label()); } }

// f(std::integral_constant<int, V>) for the V of the list that equals v, R{} (an empty KernelRef) when none
// does: turns a runtime epilogue code into a template argument.
template <class R, int... Vs, class F>
R for_value(int v, F&& f) {
  R r{};
  ((v == Vs ? (void)(r = f(std::integral_constant<int, Vs>{})) : (void)0), ...);
  return r;
}

// The C-ABI label queries: the label and its length, or -PIPNET_ERR_ARG (nothing selected, or buf too small).
template <class... Args>
int write_label(const KernelRef<Args...>& k, char* buf, int cap) {
  const std::string s = k.fn ? k.label() : "";
  if (s.empty() || !buf || (int)s.size() >= cap) return -PIPNET_ERR_ARG;
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return (int)s.size();
}

}  // namespace pipnet
