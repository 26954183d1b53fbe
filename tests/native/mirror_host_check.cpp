// CPU check of the two functions of include/tscm/tscm_calib.hpp's perception half that touch no device and call nothing
// in the library: exposure_gains (a hand-written Gaussian elimination) and rectify_pair_rotation.  The program only
// evaluates them; tests/test_cpp_mirror_host.py makes the cases and holds the answers against an exact rational solve and
// against maps.rectify_pair_rotation.  Host logic only (no GPU, no libtscm_hip).
//   usage: mirror_host_check < cases     one JSON line: {"results": [...]}, one entry per input line
//   gains n len_count len_sum sigma_n sigma_g count... sum...   -> {"gains": [...]} or {"throw": "text"}
//   rotation t1x t1y t1z t2x t2y t2z                            -> {"R": [9 values, %.17g]}
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tscm/tscm_calib.hpp"

int main()
{
    std::string line, out = "{\"results\": [";
    bool first = true;
    while (std::getline(std::cin, line)) {
        std::istringstream s(line);
        std::string what;
        if (!(s >> what)) continue;
        std::ostringstream item;
        if (what == "gains") {
            int n = 0;
            long lc = 0, ls = 0;
            double sigma_n = 0, sigma_g = 0;
            if (!(s >> n >> lc >> ls >> sigma_n >> sigma_g) || lc < 0 || ls < 0 || lc > 4096 || ls > 4096) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            std::vector<long long> count((size_t)lc), sum((size_t)ls);
            for (size_t k = 0; k < count.size(); ++k) s >> count[k];
            for (size_t k = 0; k < sum.size(); ++k) s >> sum[k];
            if (!s) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            try {
                const std::vector<unsigned short> g = tscm::exposure_gains(n, count, sum, sigma_n, sigma_g);
                item << "{\"gains\": [";
                for (size_t k = 0; k < g.size(); ++k) item << (k ? ", " : "") << g[k];
                item << "]}";
            } catch (const std::exception &e) {
                item << "{\"throw\": \"" << e.what() << "\"}";
            }
        } else if (what == "rotation") {
            double t[6];
            for (int k = 0; k < 6; ++k) s >> t[k];
            if (!s) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            const tscm::Mat33 R = tscm::rectify_pair_rotation(t, t + 3);
            item << "{\"R\": [";
            for (int k = 0; k < 9; ++k) {
                char buf[40];
                std::snprintf(buf, sizeof(buf), "%.17g", R.a[k]);
                item << (k ? ", " : "") << buf;
            }
            item << "]}";
        } else {
            std::fprintf(stderr, "bad line: %s\n", line.c_str());
            return 2;
        }
        out += (first ? "" : ", ") + item.str();
        first = false;
    }
    std::printf("%s]}\n", out.c_str());
    return 0;
}
