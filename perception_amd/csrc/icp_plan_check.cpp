// icp_plan_check.cpp - stand-alone host program (no GPU, no HIP call) around icp_plan.hpp.
//   icp_plan_check case.txt
// case.txt describes one ICP stage, one statement per line (tests/test_icp_plan_cpu.py writes it):
//   n_cu N | work_cap N | plane_on 0/1 | reject_on 0/1 | use_guess MODE | guess_frames N | batches_in_flight N | calls_in_flight N
//   device_guesses 0/1                  IcpPlanInput::device_guesses (rule C18's fine stage); when the statement is there the plan
//                                       also prints "device_guesses" and "moved_by" (guess_indexing of the plan)
//   tun NAME VALUE [VALUE VALUE]        a field of Tunables (lat_shape takes three values)
//   slot S FACES GRIDDED BIG            tpl_faces / tpl_gridded / tpl_big of template slot S
//   cluster N FRAME TPL_OFF TPL_M SLOT  one IcpCluster, in order
//   done K S                            after planning: state 2 * K + S is marked done (input of repack_active)
//   lat N_LAT LAT_MAX_N BATCHES | grid N CAP CPW CROWDED SLOTS | donate ICP_DONATE BATCHES NCL GRID | slots ICP_SLOTS BATCHES GROUPED
//   planegrid N WG_CAP | pollgroup POLLS_DONE
//                                       stand-alone queries of lat_launch_shape, whole_launch_grid, whole_donate, pipe_slots,
//                                       plane_launch_grid, sliced_poll_group
// Frame f's guess is the matrix with entries 1000 f + i, the single guess has entries -(i + 1).  The program plans the stage and
// prints every decision as one JSON object: the plan, tile0 and the initial states per cluster, the work list, and the launch
// shapes, tables and orders of the drivers the plan selects.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "icp_plan.hpp"

using namespace cd;

static void print_ints(const char* name, const int* v, int n, const char* tail = ", ") {
    std::printf("\"%s\": [", name);
    for (int i = 0; i < n; ++i) std::printf("%s%d", i ? ", " : "", v[i]);
    std::printf("]%s", tail);
}

static bool set_tunable(Tunables& t, const std::string& name, std::istringstream& ss) {
    struct Field { const char* name; int* p; };
    const Field fields[] = {{"icp_persist", &t.icp_persist}, {"icp_donate", &t.icp_donate}, {"icp_mode", &t.icp_mode}, {"icp_max_wg", &t.icp_max_wg},
                            {"icp_cpw", &t.icp_cpw}, {"icp_direct", &t.icp_direct}, {"mirror_reads", &t.mirror_reads}, {"mirror_writes", &t.mirror_writes},
                            {"icp_slots", &t.icp_slots}, {"icp_big_weight", &t.icp_big_weight}, {"icp_lattice", &t.icp_lattice}, {"copy_kernels", &t.copy_kernels}};
    if (name == "lat_shape") return (bool)(ss >> t.lat_shape[0] >> t.lat_shape[1] >> t.lat_shape[2]);
    for (const Field& f : fields) if (name == f.name) return (bool)(ss >> *f.p);
    return false;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: icp_plan_check case.txt\n"); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { std::fprintf(stderr, "icp_plan_check: cannot open %s\n", argv[1]); return 2; }
    Tunables tun;
    int tpl_faces[CD_MAX_TEMPLATES] = {0};
    bool tpl_gridded[CD_MAX_TEMPLATES] = {false}, tpl_big[CD_MAX_TEMPLATES] = {false};
    std::vector<IcpCluster> cl;
    std::vector<std::pair<int, int>> done;
    std::vector<std::string> queries;
    int n_cu = 256, work_cap = 1 << 16, plane_on = 0, use_guess = CD_GUESS_NONE, guess_frames = 0, batches = 1, calls = 1, device_guesses = -1, reject_on = -1;
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream ss(line);
        std::string key;
        if (!(ss >> key)) continue;
        bool ok = true;
        if (key == "n_cu") ok = (bool)(ss >> n_cu);
        else if (key == "work_cap") ok = (bool)(ss >> work_cap);
        else if (key == "plane_on") ok = (bool)(ss >> plane_on);
        else if (key == "use_guess") ok = (bool)(ss >> use_guess);
        else if (key == "guess_frames") ok = (bool)(ss >> guess_frames);
        else if (key == "batches_in_flight") ok = (bool)(ss >> batches);
        else if (key == "calls_in_flight") ok = (bool)(ss >> calls);
        else if (key == "device_guesses") ok = (bool)(ss >> device_guesses) && (device_guesses == 0 || device_guesses == 1);
        else if (key == "reject_on") ok = (bool)(ss >> reject_on) && (reject_on == 0 || reject_on == 1);
        else if (key == "tun") { std::string name; ok = (bool)(ss >> name) && set_tunable(tun, name, ss); }
        else if (key == "slot") {
            int s = -1, faces = 0, gridded = 0, big = 0;
            ok = (bool)(ss >> s >> faces >> gridded >> big) && s >= 0 && s < CD_MAX_TEMPLATES;
            if (ok) { tpl_faces[s] = faces; tpl_gridded[s] = gridded != 0; tpl_big[s] = big != 0; }
        } else if (key == "cluster") {
            IcpCluster c;
            std::memset(&c, 0, sizeof(c));
            ok = (bool)(ss >> c.n >> c.frame >> c.tpl_off >> c.tpl_m >> c.slot) && c.slot >= 0 && c.slot < CD_MAX_TEMPLATES && c.frame >= 0;
            c.k = (int)cl.size();
            cl.push_back(c);
        } else if (key == "done") { int k = 0, s = 0; ok = (bool)(ss >> k >> s) && k >= 0 && (s == 0 || s == 1); done.push_back({k, s}); }
        else if (key == "lat" || key == "grid" || key == "donate" || key == "slots" || key == "planegrid" || key == "pollgroup") queries.push_back(line);
        else ok = false;
        if (!ok) { std::fprintf(stderr, "icp_plan_check: cannot read \"%s\"\n", line.c_str()); return 2; }
    }
    const int ncl = (int)cl.size();
    std::vector<float> frame_guess(16 * (size_t)guess_frames);
    for (size_t i = 0; i < frame_guess.size(); ++i) frame_guess[i] = (float)(1000 * (i / 16) + i % 16);
    float icp_guess[16];
    for (int i = 0; i < 16; ++i) icp_guess[i] = -(float)(i + 1);

    std::printf("{");
    if (ncl > 0) {
        IcpPlanInput in;
        in.cl = cl.data(); in.ncl = ncl;
        in.tpl_faces = tpl_faces; in.tpl_gridded = tpl_gridded; in.tpl_big = tpl_big;
        in.tun = &tun; in.n_cu = n_cu; in.work_cap = work_cap;
        in.plane_on = plane_on != 0;
        in.icp_use_guess = use_guess;
        in.frame_guess = frame_guess.data(); in.frame_guess_len = frame_guess.size();
        in.icp_guess = icp_guess;
        if (device_guesses >= 0) in.device_guesses = device_guesses != 0;
        if (reject_on >= 0) in.reject_on = reject_on != 0;
        // (one item past the capacity, so that a planner that overruns it is caught by the sanitizer build and not by luck)
        std::vector<IcpWork> work((size_t)std::max(work_cap, 0) + 1);
        std::vector<IcpState> st(2 * (size_t)ncl);
        IcpPlan pl;
        const PlanStatus ps = plan_icp(in, &pl, work.data(), st.data());
        std::printf("\"status\": %d, \"message\": \"%s\", ", ps.code, ps.msg ? ps.msg : "");
        if (ps.code == CD_OK) {
            std::printf("\"plan\": {\"ncl\": %d, \"guess_mode\": %d, \"max_n\": %d, \"qslice\": %d, \"guess_need\": %zu, \"n_lat\": %d, \"n_live\": %d, \"lat_max_n\": %d, "
                        "\"icp_search\": %d, \"nwork\": %d, \"wg_cap\": %d, \"grouped_pipe\": %d, \"lat_direct\": %d, \"pipe_ok\": %d, \"big_ok\": %d, \"whole_cluster\": %d, \"plane\": %d, ",
                        pl.ncl, pl.guess_mode, pl.max_n, pl.qslice, pl.guess_need, pl.n_lat, pl.n_live, pl.lat_max_n, pl.icp_search, pl.nwork, pl.wg_cap,
                        (int)pl.grouped_pipe, (int)pl.lat_direct, (int)pl.pipe_ok, (int)pl.big_ok, (int)pl.whole_cluster, (int)pl.plane);
            if (device_guesses >= 0) std::printf("\"device_guesses\": %d, \"moved_by\": %d, ", (int)pl.device_guesses, guess_indexing(pl));
            if (reject_on >= 0) std::printf("\"reject\": %d, ", (int)pl.reject);
            std::vector<int> v;
            for (char x : pl.in_lat) v.push_back(x);
            print_ints("in_lat", v.data(), (int)v.size());
            std::printf("\"groups\": [");
            for (size_t g = 0; g < pl.groups.size(); ++g)
                std::printf("%s[%d, %d, %d, %d, %lld]", g ? ", " : "", pl.groups[g].beg, pl.groups[g].end, pl.groups[g].live, pl.groups[g].kind, pl.groups[g].pts);
            std::printf("]}, ");
            v.clear();
            for (const IcpCluster& c : cl) v.push_back(c.tile0);
            print_ints("tile0", v.data(), ncl);
            std::printf("\"work\": [");
            for (int w = 0; w < pl.nwork; ++w) std::printf("%s[%d, %d]", w ? ", " : "", work[(size_t)w].cluster, work[(size_t)w].tile);
            std::printf("], \"states\": [");
            for (int k = 0; k < ncl; ++k) {
                const IcpState &a = st[2 * (size_t)k], &b = st[2 * (size_t)k + 1];
                // [status of slot 0, of slot 1, done of slot 0, of slot 1, the two slots are equal byte for byte, prev_mse is DBL_MAX,
                //  Tfinal of slot 0 (0: the identity)]
                std::printf("%s[%d, %d, %d, %d, %d, %d, ", k ? ", " : "", a.status, b.status, a.done, b.done,
                            (int)(std::memcmp(&a, &b, sizeof(a)) == 0), (int)(a.prev_mse == std::numeric_limits<double>::max()));
                bool identity = true;
                for (int i = 0; i < 16; ++i) identity = identity && a.Tfinal[i] == (i % 5 == 0 ? 1.f : 0.f);
                if (identity) std::printf("0]");
                else {
                    for (int i = 0; i < 16; ++i) std::printf("%s%.9g", i ? ", " : "[", (double)a.Tfinal[i]);
                    std::printf("]]");
                }
            }
            std::printf("], ");
            // the launches, in the order stage_icp hands the clusters on
            std::vector<int> order((size_t)ncl), tab(3 * 1024);
            if (pl.n_lat > 0) {
                int no = 0;
                for (int k = 0; k < ncl; ++k) if (pl.in_lat[(size_t)k]) order[(size_t)no++] = k;
                largest_first(order.data(), no, cl.data());
                const LatShape ls = lat_launch_shape(pl.n_lat, pl.lat_max_n, batches, tun.lat_shape);
                std::printf("\"lat\": {\"cpw\": %d, \"wpc\": %d, \"per_slot\": %d, \"n_wg\": %d, ", ls.cpw, ls.wpc, ls.per_slot, ls.n_wg);
                print_ints("order", order.data(), no, "}, ");
            }
            const bool crowded = icp_crowded(batches);
            if (pl.grouped_pipe) {
                const GroupedLaunch L = grouped_launch_table(pl.groups, cl.data(), pl.wg_cap, tun, order.data(), tab.data());
                std::printf("\"grouped\": {\"big_weight\": %lld, \"n_wg\": %d, \"slots\": %d, ", L.big_weight, L.n_wg, pipe_slots(tun.icp_slots, crowded, true));
                print_ints("wg_of", L.wg_of, 3);
                print_ints("tab_of", L.tab_of, 3);
                print_ints("share", L.share, std::min(L.nq, 16));
                print_ints("order", order.data(), L.no);
                print_ints("tab", tab.data(), L.ntab, "}, ");
            }
            if (pl.whole_cluster) {
                for (int k = 0; k < ncl; ++k) order[(size_t)k] = k;
                largest_first(order.data(), ncl, cl.data());
                const int slots = pipe_slots(tun.icp_slots, crowded, false), grid = whole_launch_grid(ncl, pl.wg_cap, tun.icp_cpw, crowded, slots);
                std::printf("\"whole\": {\"slots\": %d, \"grid\": %d, \"donate\": %d, ", slots, grid, (int)((pl.pipe_ok || pl.big_ok) && whole_donate(tun.icp_donate, batches, ncl, grid)));
                print_ints("order", order.data(), ncl, "}, ");
            }
            const PersistLaunch pe = persist_launch(cl.data(), ncl, pl.nwork, pl.wg_cap, tun.icp_persist, calls);
            std::printf("\"persist\": {\"launch\": %d, \"G\": %d, \"n_open\": %d}, ", (int)pe.launch, pe.G, pe.n_open);
            for (const auto& d : done) if (d.first < ncl) st[2 * (size_t)d.first + (size_t)d.second].done = 1;
            std::vector<IcpWork> active((size_t)std::max(pl.nwork, 1));
            bool all = false;
            const int na = repack_active(work.data(), pl.nwork, st.data(), ncl, active.data(), &all);
            std::printf("\"repack\": {\"all_done\": %d, \"active\": [", (int)all);
            for (int w = 0; w < na; ++w) std::printf("%s[%d, %d]", w ? ", " : "", active[(size_t)w].cluster, active[(size_t)w].tile);
            std::printf("]}, ");
        }
    }
    std::printf("\"queries\": [");
    for (size_t q = 0; q < queries.size(); ++q) {
        std::istringstream ss(queries[q]);
        std::string key;
        int a[5] = {0, 0, 0, 0, 0};
        ss >> key;
        for (int& x : a) ss >> x;
        std::printf("%s", q ? ", " : "");
        if (key == "lat") {
            const LatShape ls = lat_launch_shape(a[0], a[1], a[2], tun.lat_shape);
            std::printf("[%d, %d, %d, %d]", ls.cpw, ls.wpc, ls.per_slot, ls.n_wg);
        } else if (key == "grid") std::printf("%d", whole_launch_grid(a[0], a[1], a[2], a[3] != 0, a[4]));
        else if (key == "donate") std::printf("%d", (int)whole_donate(a[0], a[1], a[2], a[3]));
        else if (key == "planegrid") std::printf("%d", plane_launch_grid(a[0], a[1]));
        else if (key == "pollgroup") std::printf("%d", sliced_poll_group(a[0]));
        else std::printf("%d", pipe_slots(a[0], icp_crowded(a[1]), a[2] != 0));
    }
    std::printf("]}\n");
    return 0;
}
