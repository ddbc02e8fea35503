// CPU build of the general-nu Matern routine (csrc/matern_dev.h): reads "nu t" pairs from stdin, prints
// "t^nu K_nu(t)  t^nu K_(nu-1)(t)  k(r = t / sqrt(2 nu))" per line (tests/test_matern_nu_host.py compares with scipy)
#include <cstdio>

#include "../../bayesian-inference_amd/csrc/matern_dev.h"

int main() {
  double nu, t;
  while (std::scanf("%lf %lf", &nu, &t) == 2) {
    const gpemu::MaternNu c = gpemu::matern_nu_constants(nu);
    double kn, km;
    gpemu::matern_nu_bessel(c, t, kn, km);
    std::printf("%.17e %.17e %.17e\n", kn, km, gpemu::matern_nu_value(c, t / c.s2nu));
  }
  return 0;
}
