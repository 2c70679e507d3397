// Host build of csrc/range_scale.h (tests/test_range_scale.py): the exponents the double-precision entry points rescale by,
// over the whole double range -- every binade from the smallest subnormal to DBL_MAX, several mantissas in each, the powers
// of two, the binade edges and DBL_MAX itself.  Prints "ok <count>" or the first failing maximum.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../flucoma-core_amd/csrc/range_scale.h"

static bool check(double m)
{
  using namespace fluhip;
  const int e = nmf_range_exponent(m);
  if (m <= 0x1p128)
  {
    if (e != 0) return false;
  }
  else
  {
    const double s = std::ldexp(m, -e);
    // scaled to <= 2^128 exactly (a power of two: the mantissa is kept) and by the smallest such power
    if (!(e > 0 && s <= 0x1p128 && std::ldexp(s, 1) > 0x1p128 && std::ldexp(s, e) == m)) return false;
  }
  const int f = svd_range_exponent(m);
  const double t = std::ldexp(m, -f);
  return t >= 0.5 && t < 1.0 && std::ldexp(t, f) == m;
}

int main()
{
  std::vector<double> xs = {DBL_MAX, std::nextafter(DBL_MAX, 0.0), DBL_MIN, std::nextafter(DBL_MIN, 0.0), DBL_TRUE_MIN,
                            0x1p128, std::nextafter(0x1p128, 0.0), std::nextafter(0x1p128, INFINITY), 0x1p129, 1.0};
  const double mant[] = {1.0, 1.0000000000000002, 1.25, 1.5, 1.9999999999999998};
  for (int b = -1074; b <= 1023; b++)
    for (double mt : mant)
    {
      const double x = std::ldexp(mt, b);
      if (x > 0 && std::isfinite(x)) xs.push_back(x);
    }
  for (double x : xs)
    if (!check(x))
    {
      std::printf("fail %.17g %d %d\n", x, fluhip::nmf_range_exponent(x), fluhip::svd_range_exponent(x));
      return 1;
    }
  const bool edges = fluhip::nmf_range_exponent(DBL_MAX) == 1024 - 128 && fluhip::nmf_range_exponent(0x1p128) == 0 &&
                     fluhip::nmf_range_exponent(0x1p129) == 1 && fluhip::nmf_range_exponent(DBL_TRUE_MIN) == 0 &&
                     fluhip::svd_range_exponent(DBL_TRUE_MIN) == -1073 && fluhip::svd_range_exponent(0.0) == 0;
  if (!edges)
  {
    std::printf("fail edges\n");
    return 1;
  }
  std::printf("ok %zu\n", xs.size());
  return 0;
}
