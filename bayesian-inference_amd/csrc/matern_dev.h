// Matern kernel of general smoothness nu (sklearn's general branch, skl kernels.py:1725-1733 values, 1767-1774
// gradients): for one scaled distance t = sqrt(2 nu) r
//     k(t) = 2^(1 - nu) / Gamma(nu) t^nu K_nu(t)          d/dt [t^nu K_nu(t)] = -t^nu K_(nu-1)(t)
// with K the modified Bessel function of the second kind.
//
// nu = mu + n (n = round(nu), |mu| <= 1/2; for nu < 1/2: mu = -nu, see below).  K_mu and K_(mu+1) come from
//   t <= 2   Temme's series (N. M. Temme, J. Comput. Phys. 19 (1975) 324):
//              K_mu = sum_k c_k f_k,  K_(mu+1) = 2/t sum_k c_k (p_k - k f_k),  c_k = (t^2/4)^k / k!
//              f_0 = mu pi / sin(mu pi) [cosh(s) G1(mu) + sinh(s)/s ln(2/t) G2(mu)],  s = mu ln(2/t)
//              p_0 = 1/2 (t/2)^-mu Gamma(1 + mu),  q_0 = 1/2 (t/2)^mu Gamma(1 - mu)
//              f_k = (k f_(k-1) + p_(k-1) + q_(k-1)) / (k^2 - mu^2),  p_k = p_(k-1) / (k - mu),  q_k = q_(k-1) / (k + mu)
//              G1(mu) = (1/Gamma(1 - mu) - 1/Gamma(1 + mu)) / (2 mu),  G2(mu) = (1/Gamma(1 - mu) + 1/Gamma(1 + mu)) / 2
//   t > 2    Steed's continued fraction in the Thompson-Barnett form (I. J. Thompson, A. R. Barnett, J. Comput.
//            Phys. 64 (1986) 490), scaled by e^t: K_mu e^t = sqrt(pi / 2t) / S with S the sum of the series that
//            accompanies the continued fraction, so that the factor e^-t is applied once, at the end (a large t
//            gives 0, never 0 * inf)
// then the upward recurrence K_(v+1) = K_(v-1) + 2v/t K_v to K_(nu-1), K_nu.  For nu < 1/2 (n = 0) the pair is
// taken at mu = -nu: (K_-nu, K_(1-nu)) = (K_nu, K_(nu-1)), no recurrence.
//
// Everything that depends on nu alone is formed on the host once per model / fit handle (matern_nu_constants) and
// handed to the kernels by value; the device runs only the loops.  Fixed trip count of the series (Guideline 5:
// every lane of a wave in the t <= 2 branch runs the same 16 terms); the continued fraction stops on convergence.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GPEMU_HD __host__ __device__
#else
#define GPEMU_HD
#endif

namespace gpemu {

struct MaternNu {
  double nu;          // smoothness
  double mu;          // base order of the pair (K_mu, K_(mu+1)), |mu| <= 1/2
  double fact;        // mu pi / sin(mu pi)
  double gam1, gam2;  // G1(mu), G2(mu)
  double gampl, gammi;  // 1 / Gamma(1 + mu), 1 / Gamma(1 - mu)
  double pref;        // 2^(1 - nu) / Gamma(nu)
  double s2nu;        // sqrt(2 nu): t = s2nu r
  int nrec;           // upward recurrence steps from (K_mu, K_(mu+1)) to (K_(nu-1), K_nu)
  int swap;           // 1: (K_mu, K_(mu+1)) already is (K_nu, K_(nu-1))
};

// host: the constants of one nu (finite, > 0)
inline MaternNu matern_nu_constants(double nu) {
  MaternNu c{};
  c.nu = nu;
  const double n = std::nearbyint(nu);
  if (n == 0.0) {
    c.mu = -nu;
    c.nrec = 0;
    c.swap = 1;
  } else {
    c.mu = nu - n;
    c.nrec = (int)n - 1;
    c.swap = 0;
  }
  const long double mu = c.mu;
  const long double pi = 3.141592653589793238462643383279503L;
  c.fact = (mu == 0.0L) ? 1.0 : (double)(mu * pi / std::sin(mu * pi));
  if (std::fabs((double)mu) < 1e-3) {
    // 1/Gamma(1 + z) = sum_k a_(k+1) z^k (Abramowitz & Stegun 6.1.34): G1 = -(a2 + a4 mu^2 + a6 mu^4 + a8 mu^6),
    // G2 = a1 + a3 mu^2 + a5 mu^4 + a7 mu^6
    const long double m2 = mu * mu;
    c.gam1 = (double)-(0.5772156649015328606L + m2 * (-0.0420026350340952355L + m2 * (-0.0421977345555443367L +
                                                                                     m2 * 0.0072189432466630995L)));
    c.gam2 = (double)(1.0L + m2 * (-0.6558780715202538811L + m2 * (0.1665386113822914895L +
                                                                  m2 * -0.0096219715278769736L)));
    c.gampl = (double)(1.0L / std::tgamma(1.0L + mu));
    c.gammi = (double)(1.0L / std::tgamma(1.0L - mu));
  } else {
    const long double gp = 1.0L / std::tgamma(1.0L + mu), gm = 1.0L / std::tgamma(1.0L - mu);
    c.gam1 = (double)((gm - gp) / (2.0L * mu));
    c.gam2 = (double)((gm + gp) / 2.0L);
    c.gampl = (double)gp;
    c.gammi = (double)gm;
  }
  c.pref = (double)(std::exp2((long double)(1.0 - nu)) / std::tgamma((long double)nu));
  c.s2nu = std::sqrt(2.0 * nu);
  return c;
}

constexpr int MATERN_TEMME_TERMS = 16;   // t <= 2: term k ~ 1 / (k!)^2 relative to the sum; 16! ^2 ~ 4e26
constexpr int MATERN_CF_MAX = 200;       // t > 2: converges in < 60 steps at t = 2, fewer beyond

// t^nu K_nu(t) and t^nu K_(nu-1)(t) for t > 0
GPEMU_HD inline void matern_nu_bessel(const MaternNu &c, double t, double &tk_nu, double &tk_num1) {
  const double mu = c.mu;
  double k0, k1, scale;   // K_mu, K_(mu+1) (times e^t for t > 2); the factor that undoes the scaling
  if (t <= 2.0) {
    const double lg = -log(0.5 * t);       // ln(2/t)
    const double s = mu * lg;
    const double shs = (s == 0.0) ? 1.0 : sinh(s) / s;
    double f = c.fact * (c.gam1 * cosh(s) + c.gam2 * shs * lg);
    const double es = exp(s);              // (t/2)^-mu
    double p = 0.5 * es / c.gampl, q = 0.5 / (es * c.gammi);
    const double x2 = 0.25 * t * t;
    double ck = 1.0, sum = f, sum1 = p;
#pragma unroll 4
    for (int i = 1; i <= MATERN_TEMME_TERMS; ++i) {
      const double di = (double)i;
      f = (di * f + p + q) / (di * di - mu * mu);
      ck *= x2 / di;
      p /= (di - mu);
      q /= (di + mu);
      sum = fma(ck, f, sum);
      sum1 = fma(ck, p - di * f, sum1);
    }
    k0 = sum;
    k1 = sum1 * 2.0 / t;
    scale = 1.0;
  } else {
    double b = 2.0 * (1.0 + t), d = 1.0 / b, h = d, delh = d;
    double q1 = 0.0, q2 = 1.0;
    const double a1 = 0.25 - mu * mu;
    double q = a1, cc = a1, a = -a1;
    double s = fma(q, delh, 1.0);
    for (int i = 2; i <= MATERN_CF_MAX; ++i) {
      a -= 2.0 * (i - 1);
      cc = -a * cc / i;
      const double qn = (q1 - b * q2) / a;
      q1 = q2;
      q2 = qn;
      q = fma(cc, qn, q);
      b += 2.0;
      d = 1.0 / fma(a, d, b);
      delh = (b * d - 1.0) * delh;
      h += delh;
      const double dels = q * delh;
      s += dels;
      if (fabs(dels) < 1.0e-17 * fabs(s)) break;
    }
    h = a1 * h;
    k0 = sqrt(1.5707963267948966 / t) / s;
    k1 = k0 * (mu + t + 0.5 - h) / t;
    scale = exp(-t);
  }
  // upward to (K_(nu-1), K_nu)
  double v = mu + 1.0;
  for (int i = 0; i < c.nrec; ++i) {
    const double k2 = fma(2.0 * v / t, k1, k0);
    k0 = k1;
    k1 = k2;
    v += 1.0;
  }
  const double tn = pow(t, c.nu);
  if (c.swap) {
    tk_nu = (tn * k0) * scale;
    tk_num1 = (tn * k1) * scale;
  } else {
    tk_nu = (tn * k1) * scale;
    tk_num1 = (tn * k0) * scale;
  }
}

// the kernel value from the unscaled distance r (skl: 1 at r = 0)
GPEMU_HD inline double matern_nu_value(const MaternNu &c, double r) {
  if (r == 0.0) return 1.0;
  double kn, km;
  matern_nu_bessel(c, c.s2nu * r, kn, km);
  return c.pref * kn;
}

// value and f = -(1/r) dk/dr, so that dk/dlog l_dd = f (x - x')_dd^2 / l_dd^2 (0 at r = 0, where the derivative of the
// summand vanishes): dk/dr = -pref sqrt(2 nu) t^nu K_(nu-1)(t)  ->  f = pref 2 nu t^nu K_(nu-1)(t) / t
GPEMU_HD inline double matern_nu_value_grad(const MaternNu &c, double r, double &f) {
  if (r == 0.0) {
    f = 0.0;
    return 1.0;
  }
  const double t = c.s2nu * r;
  double kn, km;
  matern_nu_bessel(c, t, kn, km);
  f = c.pref * 2.0 * c.nu * km / t;
  return c.pref * kn;
}

#if defined(__HIPCC__)
// the closed forms from the squared scaled distance r2: kind 0 RBF, 1 / 2 / 3 Matern 0.5 / 1.5 / 2.5 (internal.h:
// base_kind; kind 4 is matern_nu_value above).  Each caller forms r2 in its own way (the bits differ between the forms).
__device__ __forceinline__ double base_from_r2(int kind, double r2) {
  if (kind == 0) return exp(-0.5 * r2);
  double r = sqrt(r2);
  if (kind == 1) return exp(-r);
  if (kind == 2) {
    double t = r * 1.7320508075688772;
    return (1.0 + t) * exp(-t);
  }
  double t = r * 2.23606797749979;
  return (1.0 + t + t * t / 3.0) * exp(-t);
}

// The cross-kernel's call (predict_dev.h: kstar_value4, four values per lane and tile): one out-of-line copy of the
// Bessel loops instead of one inlined per accumulator register (kstar_kernel<4, 2, 2, 2>: ~20 000 instructions inlined,
// beyond the instruction cache).  -DGPEMU_MATERN_NU_INLINE inlines it again (A/B: tools/time_matern_nu.py).
#ifdef GPEMU_MATERN_NU_INLINE
__device__ __forceinline__
#else
__device__ __noinline__
#endif
double matern_nu_value_call(const MaternNu c, double r) {
  return matern_nu_value(c, r);
}
#endif

}  // namespace gpemu
