// The modified Bessel function of the Kaiser windows that the host-side table fills share (xover.hip, truepeak.hip, rateconv.hip).
#pragma once

namespace p2phd {

// I0(x), x >= 0: the power series sum_m ((x / 2)^2m / (m!)^2), every term positive; stops when a term no longer changes the sum
inline double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int m = 1; m < 1000; ++m) {
    term *= q / ((double)m * (double)m);
    const double next = sum + term;
    if (next == sum) break;
    sum = next;
  }
  return sum;
}

}  // namespace p2phd
