/* oracle/refshim/cudavec: stand-in for the main-repo opencv2/core/cuda/functional.hpp -- the functor bases.  TEST INFRASTRUCTURE. */
#ifndef ORACLE_CUDASHIM_FUNCTIONAL_HPP
#define ORACLE_CUDASHIM_FUNCTIONAL_HPP
namespace cv { namespace cuda { namespace device {
template <typename A, typename R> struct unary_function { typedef A argument_type; typedef R result_type; };
template <typename A1, typename A2, typename R> struct binary_function { typedef A1 first_argument_type; typedef A2 second_argument_type; typedef R result_type; };
template <typename T> struct plus : binary_function<T, T, T> { T operator()(const T &a, const T &b) const { return a + b; } };
}}}
#endif
