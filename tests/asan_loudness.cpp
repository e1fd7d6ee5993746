// Sanitizer run of the loudness meter's host side on random projects (built by tests/test_loudness_host.py with g++
// -fsanitize=address,undefined against tests/mock_hip.cpp + tests/mock_stems.cpp + tests/mock_loudness.cpp -- no GPU, nothing
// computed): every project renders through its State's graph with its stems set, at 16 and 24 bits, resampled and not, and is
// measured with td_graph_loudness (the output and every stem), td_graph_momentary, and -- stems cleared -- td_batch_loudness.
//   usage: asan_loudness <dir> ...     each <dir> holds project.lua, meta.txt ("<buffer length>") and stems.txt (one name per line)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "termdaw_amd.h"

extern size_t g_loud_launches, g_loud_signals, g_loud_hops;

static std::string slurp(const std::string& p) {
    std::string s; FILE* f = fopen(p.c_str(), "rb"); if (!f) return s;
    char b[4096]; size_t n; while ((n = fread(b, 1, sizeof b, f)) > 0) s.append(b, n); fclose(f); return s;
}
int main(int argc, char** argv) {
    size_t measured = 0, rejected = 0, failed = 0;
    for (int a = 1; a < argc; ++a) {
        const std::string dir = argv[a];
        const std::string lua = slurp(dir + "/project.lua");
        const size_t bl = (size_t)atol(slurp(dir + "/meta.txt").c_str());
        std::vector<std::string> stems;
        {
            const std::string t = slurp(dir + "/stems.txt");
            size_t at = 0;
            while (at < t.size()) {
                size_t e = t.find('\n', at);
                if (e == std::string::npos) e = t.size();
                if (e > at) stems.push_back(t.substr(at, e - at));
                at = e + 1;
            }
        }
        if (lua.empty() || !bl || stems.empty()) { fprintf(stderr, "bad project dir %s\n", dir.c_str()); return 2; }
        std::vector<const char*> names;
        for (auto& s : stems) names.push_back(s.c_str());
        td_state* s = td_state_new(dir.c_str(), 48000, bl);
        if (!s) return 3;
        if (!td_state_refresh_source(s, lua.c_str())) { ++rejected; td_state_free(s); continue; }
        td_graph* g = td_state_graph(s);
        std::vector<double> out(8 * (names.size() + 2));
        if (td_graph_loudness(g, out.data(), 1) || !strstr(td_last_error(), "no whole render")) ++failed;   // (nothing rendered yet)
        if (!td_graph_set_stems(g, names.data(), names.size())) ++failed;
        const size_t cs = td_state_chunk_count(s);
        for (int k = 0; k < 3; ++k) {
            size_t n = 0;
            if (k == 0) n = td_graph_render_all(g, td_state_samplebank(s), td_state_flowwbank(s), cs, 16);
            if (k == 1) n = td_graph_render_all(g, td_state_samplebank(s), td_state_flowwbank(s), cs, 24);
            if (k == 2) n = td_graph_render_all_resampled(g, td_state_samplebank(s), td_state_flowwbank(s), cs, 8, 48000, 44100);
            if (!n && cs) { ++failed; fprintf(stderr, "%s: %s\n", dir.c_str(), td_last_error()); continue; }
            td_graph_set_time(g, 0);
            td_flowwbank_set_time(td_state_flowwbank(s), 0);
            td_graph_reset_normalize_vertices(g);
            if (!cs) continue;
            if (!td_graph_loudness(g, out.data(), names.size() + 1)) { ++failed; fprintf(stderr, "%s: %s\n", dir.c_str(), td_last_error()); }
            if (td_graph_loudness(g, out.data(), names.size() + 2)) ++failed;   // (one more signal than the render has)
            for (size_t i = 0; i <= names.size(); ++i) {
                if (out[8 * i + 6] != (double)n || out[8 * i + 7] != (k == 2 ? 44100.0 : 48000.0)) ++failed;
                std::vector<double> m(td_graph_momentary(g, i, nullptr, 0) + 1);
                if (td_graph_momentary(g, i, m.data(), m.size()) + 1 != m.size()) ++failed;
            }
            if (td_graph_momentary(g, names.size() + 1, nullptr, 0)) ++failed;
            ++measured;
        }
        if (cs) {   // a batch of the project (stems cleared: batches refuse them)
            if (!td_graph_set_stems(g, nullptr, 0)) ++failed;
            td_batch* b = td_batch_new();
            if (td_batch_add(b, g, td_state_samplebank(s), td_state_flowwbank(s)) < 0) ++failed;
            if (!td_batch_render_all(b, cs, 16)) ++failed;
            if (!td_batch_loudness(b, out.data())) { ++failed; fprintf(stderr, "%s: %s\n", dir.c_str(), td_last_error()); }
            td_batch_free(b);
            ++measured;
        }
        td_state_free(s);
    }
    printf("asan_loudness done: %d projects, %zu measurements, %zu rejected refreshes, %zu failed calls; "
           "k_loudness launches %zu (%zu signals, %zu hops)\n",
           argc - 1, measured, rejected, failed, g_loud_launches, g_loud_signals, g_loud_hops);
    return failed ? 1 : 0;
}
