// icp_coarse_plan_check.cpp - stand-alone host program (no GPU, no HIP call) around icp_coarse_plan.hpp.
//   icp_coarse_plan_check case.txt
// case.txt describes one ICP stage and stand-alone queries, one statement per line (tests/test_icp_coarse_cpu.py writes it):
//   setting STRIDE MIN_POINTS | capacity POINTS
//   cluster N SRC_OFF TPL_M SLOT FRAME     one IcpCluster of the stage, in order (tpl_off = 1000 * SLOT)
//   state STATUS CONVERGED T0 .. T15       a final coarse state for coarse_handover (nan, inf, -inf are read)
//   subsample N STRIDE MIN_POINTS CAPACITY a call of coarse_subsample into a buffer of exactly CAPACITY ints
//   ok STRIDE MIN_POINTS                   coarse_setting_ok
// The program plans the stage and prints every output as one JSON object.  The buffers it hands out are exactly as large as it
// says, so that the sanitizer build catches a planner that overruns them.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "icp_coarse_plan.hpp"

using namespace cd;

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: icp_coarse_plan_check case.txt\n"); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { std::fprintf(stderr, "icp_coarse_plan_check: cannot open %s\n", argv[1]); return 2; }
    int stride = 0, min_points = 0;
    long long capacity = 0;
    std::vector<IcpCluster> cl;
    struct State { int status, converged; float T[16]; };
    std::vector<State> states;
    struct Sub { int n, stride, min_points, capacity; };
    std::vector<Sub> subs;
    std::vector<std::pair<int, int>> oks;
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream ss(line);
        std::string key;
        if (!(ss >> key)) continue;
        bool ok = true;
        if (key == "setting") ok = (bool)(ss >> stride >> min_points);
        else if (key == "capacity") ok = (bool)(ss >> capacity);
        else if (key == "cluster") {
            IcpCluster c;
            std::memset(&c, 0, sizeof(c));
            ok = (bool)(ss >> c.n >> c.src_off >> c.tpl_m >> c.slot >> c.frame);
            c.tpl_off = 1000 * c.slot;
            c.k = (int)cl.size();
            c.tile0 = 7;   // (a coarse problem starts its work list anew)
            cl.push_back(c);
        } else if (key == "state") {
            State s;
            ok = (bool)(ss >> s.status >> s.converged);
            for (int i = 0; i < 16 && ok; ++i) {
                std::string tok;
                ok = (bool)(ss >> tok);
                if (ok) s.T[i] = std::strtof(tok.c_str(), nullptr);
            }
            states.push_back(s);
        } else if (key == "subsample") { Sub s; ok = (bool)(ss >> s.n >> s.stride >> s.min_points >> s.capacity) && s.capacity >= 0; subs.push_back(s); }
        else if (key == "ok") { int a = 0, b = 0; ok = (bool)(ss >> a >> b); oks.push_back({a, b}); }
        else ok = false;
        if (!ok) { std::fprintf(stderr, "icp_coarse_plan_check: cannot read \"%s\"\n", line.c_str()); return 2; }
    }
    CoarsePlan pl;
    const int status = plan_coarse(cl.data(), (int)cl.size(), stride, min_points, capacity, &pl);
    std::printf("{\"status\": %d, \"n_eligible\": %d, \"max_n_coarse\": %d, \"region_begin\": %lld, \"capacity_needed\": %lld, \"coarse\": [", status,
                pl.n_eligible, pl.max_n_coarse, pl.region_begin, pl.capacity_needed);
    for (size_t j = 0; j < pl.coarse.size(); ++j) {
        const IcpCluster& c = pl.coarse[j];
        std::printf("%s[%d, %d, %d, %d, %d, %d, %d, %d]", j ? ", " : "", c.src_off, c.n, c.frame, c.k, c.tpl_off, c.tpl_m, c.tile0, c.slot);
    }
    std::printf("], \"gather\": [");
    for (size_t j = 0; j < pl.gather.size(); ++j)
        std::printf("%s[%d, %d, %d, %d]", j ? ", " : "", pl.gather[j].src_off, pl.gather[j].dst_off, pl.gather[j].n_coarse, pl.gather[j].stride);
    std::printf("], \"hand\": [");
    for (size_t k = 0; k < pl.hand.size(); ++k) std::printf("%s[%d, %d]", k ? ", " : "", pl.hand[k].coarse, pl.hand[k].n_coarse);
    std::printf("], \"handover\": [");
    for (size_t i = 0; i < states.size(); ++i) {
        int fb = -1;
        const int st = coarse_handover(states[i].status, states[i].converged, states[i].T, &fb);
        std::printf("%s[%d, %d]", i ? ", " : "", st, fb);
    }
    std::printf("], \"subsample\": [");
    for (size_t i = 0; i < subs.size(); ++i) {
        std::vector<int32_t> out((size_t)subs[i].capacity);   // exactly the capacity: one index too many is a heap overflow
        const int n = coarse_subsample(subs[i].n, subs[i].stride, subs[i].min_points, out.data(), subs[i].capacity);
        std::printf("%s[%d", i ? ", " : "", n);
        for (int j = 0; j < n && n <= subs[i].capacity; ++j) std::printf(", %d", out[(size_t)j]);
        std::printf("]");
    }
    std::printf("], \"ok\": [");
    for (size_t i = 0; i < oks.size(); ++i) std::printf("%s%d", i ? ", " : "", (int)coarse_setting_ok(oks[i].first, oks[i].second));
    std::printf("]}\n");
    return 0;
}
