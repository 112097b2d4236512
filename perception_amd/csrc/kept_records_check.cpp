// kept_records_check.cpp - stand-alone host program (no GPU, no HIP header) around kept_records.hpp.
//   kept_records_check script.txt
// script.txt drives one KeptRecords of a small POD, one statement per line (tests/test_kept_records_cpu.py writes it):
//   begin NCL                      begin(NCL)
//   keep K ID                      keep(K, mirror record ID)
//   assign ID ...                  assign_all over the listed mirror records (none: n = 0, a null source)
//   publish FIRST ...              publish(the index)
//   single ID                      publish_single(mirror record ID)
//   invalidate
//   read FRAME FIRST COUNT [null]  read into a buffer of exactly COUNT records (null: no buffer)
// Mirror record ID is {ID, ID + 0.5}.  Every read prints [its return, [the ids written], every record written is whole (its value
// is its id + 0.5, or it is an all-zero default record) and the rest of the buffer untouched, valid()] as one element of a JSON list.  The buffers are exactly as large as the call says, so that the sanitizer build catches a read that
// overruns them.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "kept_records.hpp"

struct Rec { int32_t id; float v; };      // what the API hands out
struct Mirror { int32_t id; float v; };   // the same layout under the kernels' name

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: kept_records_check script.txt\n"); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { std::fprintf(stderr, "kept_records_check: cannot open %s\n", argv[1]); return 2; }
    cd::KeptRecords<Rec> kept;
    std::string line;
    bool any = false;
    std::printf("[");
    while (std::getline(file, line)) {
        std::istringstream ss(line);
        std::string key;
        if (!(ss >> key)) continue;
        std::vector<int> v;
        for (int x; ss >> x;) v.push_back(x);
        std::string tail;
        ss.clear();
        ss >> tail;
        const size_t n = v.size();
        bool ok = tail.empty();
        if (key == "begin" && n == 1) kept.begin(v[0]);
        else if (key == "keep" && n == 2) kept.keep(v[0], Mirror{v[1], (float)v[1] + 0.5f});
        else if (key == "assign") {
            std::vector<Mirror> src;
            for (int id : v) src.push_back(Mirror{id, (float)id + 0.5f});
            kept.assign_all(src.empty() ? (const Mirror*)nullptr : src.data(), (int)src.size());
        } else if (key == "publish") kept.publish(v);
        else if (key == "single" && n == 1) kept.publish_single(Mirror{v[0], (float)v[0] + 0.5f});
        else if (key == "invalidate" && n == 0) kept.invalidate();
        else if (key == "read" && n == 3) {
            ok = tail.empty() || tail == "null";
            std::vector<Rec> out((size_t)std::max(v[2], 0), Rec{-1, -1.f});   // exactly the count: one record too many is a heap overflow
            const int got = kept.read(v[0], v[1], v[2], tail == "null" || out.empty() ? nullptr : out.data());
            bool values = true;
            std::printf("%s[%d, [", any ? ", " : "", got);
            for (int i = 0; i < got; ++i) {
                std::printf("%s%d", i ? ", " : "", out[(size_t)i].id);
                const Rec& r = out[(size_t)i];
                values = values && (r.v == (float)r.id + 0.5f || (r.id == 0 && r.v == 0.f));   // (a default record: all zero)
            }
            for (size_t i = (size_t)std::max(got, 0); i < out.size(); ++i) values = values && out[i].id == -1;   // the rest is untouched
            std::printf("], %d, %d]", (int)values, (int)kept.valid());
            any = true;
        } else ok = false;
        if (!ok) { std::fprintf(stderr, "kept_records_check: cannot read \"%s\"\n", line.c_str()); return 2; }
    }
    std::printf("]\n");
    return 0;
}
