// The summary of the geodesic's profile (include/dotsocp.h: dotsocp_geodesic): the eleven layer sums of k_geodesic and the
// layers' maxima turned into scalars, in ONE stated order -- plain host C++ without HIP, shared by the library
// (Solver::geodesic_profile) and a stand-alone test program (tests/san/geodesic_summary_check.cpp); geodesic.summarize()
// restates it operation for operation, and a test holds the two bit for bit.
//
// Every product, sum and quotient below is one rounded IEEE double operation in the order written (build without
// contraction: -ffp-contract=off).
// NaN rule, stated once: every maximum / minimum is keep_max / keep_min -- `(d > m || d != d) ? d : m` resp. `<` --, which
// takes a NaN when it meets one and keeps it from then on (no later comparison with a NaN is true); a guard written
// `c > 0 ? a : b` takes `b` for a NaN c.  So a NaN layer sum shows in every scalar formed from it, except that
// speed_spread is 0 for a NaN cost.
#pragma once
#include <cmath>
#include <vector>

#include "../../include/dotsocp.h"

namespace dotsocp {

enum { GEO_MASS = 0, GEO_MX, GEO_MY, GEO_MXX, GEO_MYY, GEO_MXY, GEO_PX, GEO_PY, GEO_KIN, GEO_ENT, GEO_SQ };

inline double geo_keep_max(double m, double d) { return (d > m || d != d) ? d : m; }
inline double geo_keep_min(double m, double d) { return (d < m || d != d) ? d : m; }

// sums: the layer sums as added on the device, quantity q of layer t at sums[t + nt * q]; rho_max: nt; n_layer_nodes = ny * nx.
// mean (nt x DOTSOCP_GEO_SUMS in the same layout, or nullptr) <- every layer sum divided by (double)n_layer_nodes.
inline void geodesic_summarize(long long nt, long long n_layer_nodes, const double *sums, const double *rho_max,
                               dotsocp_geodesic *res, double *mean = nullptr) {
    const double N = (double)n_layer_nodes;
    std::vector<double> own;
    if (!mean) {
        own.resize((size_t)(nt * DOTSOCP_GEO_SUMS));
        mean = own.data();
    }
    for (long long k = 0; k < nt * DOTSOCP_GEO_SUMS; ++k) mean[k] = sums[k] / N;
    auto a = [&](int q, long long t) { return mean[t + nt * q]; };
    res->nt = nt;
    res->n_nodes = n_layer_nodes * nt;
    double cost = 0.0;
    for (long long t = 0; t < nt; ++t) cost += sums[t + nt * GEO_KIN];          // the report's formula, its order
    res->cost = cost / (double)res->n_nodes;
    double emin = a(GEO_KIN, 0), emax = a(GEO_KIN, 0);
    for (long long t = 1; t < nt; ++t) {
        emin = geo_keep_min(emin, a(GEO_KIN, t));
        emax = geo_keep_max(emax, a(GEO_KIN, t));
    }
    res->energy_min = emin;
    res->energy_max = emax;
    res->speed_spread = res->cost > 0 ? (emax - emin) / res->cost : 0.0;
    const long long e = nt - 1;
    const double cx0 = a(GEO_MX, 0) / a(GEO_MASS, 0), cy0 = a(GEO_MY, 0) / a(GEO_MASS, 0);
    const double cx1 = a(GEO_MX, e) / a(GEO_MASS, e), cy1 = a(GEO_MY, e) / a(GEO_MASS, e);
    const double gx = a(GEO_MX, e) - a(GEO_MX, 0), gy = a(GEO_MY, e) - a(GEO_MY, 0);
    double com = 0.0, mom = 0.0, peak = rho_max[0];
    long long bad = 0;
    for (long long t = 0; t < nt; ++t) {
        const double s = (double)t / (double)(nt - 1);
        const double cx = a(GEO_MX, t) / a(GEO_MASS, t), cy = a(GEO_MY, t) / a(GEO_MASS, t);
        const double dx = cx - ((1 - s) * cx0 + s * cx1), dy = cy - ((1 - s) * cy0 + s * cy1);
        com = geo_keep_max(com, std::sqrt(dx * dx + dy * dy));
        const double ex = a(GEO_PX, t) - gx, ey = a(GEO_PY, t) - gy;
        mom = geo_keep_max(mom, std::sqrt(ex * ex + ey * ey));
        peak = geo_keep_max(peak, rho_max[t]);
        if (!std::isfinite(a(GEO_MASS, t))) ++bad;
    }
    res->com_defect = com;
    res->momentum_defect = mom;
    double ent = 0.0;
    for (long long t = 1; t + 1 < nt; ++t)
        ent = geo_keep_max(ent, -((a(GEO_ENT, t - 1) + a(GEO_ENT, t + 1)) - 2 * a(GEO_ENT, t)));
    res->entropy_defect = ent;
    res->peak_excess = geo_keep_max(0.0, peak - geo_keep_max(rho_max[0], rho_max[e]));
    res->nonfinite = bad;
}

}  // namespace dotsocp
