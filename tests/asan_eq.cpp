// Sanitizer run of the EQ vertex' host side (built by tests/test_eq_host.py with g++ -fsanitize=address,undefined against
// tests/mock_hip.cpp + tests/mock_eq.cpp -- no GPU, nothing computed): every project
// goes through the front-end and the C ABI in every band mode with sine modes 1 and 2, un-chunked and in 4 096-frame chunks --
// fresh, scanned and continued renders, block pulls, a set_time in between, a batch of the project with a second copy of
// itself.  Per project it prints the launch families one profiled render under the guard modes went through ("launches <dir>:
// name=count ...") and the static gain the guard carried from its last guarded launch to the output ("guard <dir>: path=..."),
// which is what the guard-rule and launch-list tests read.
//   usage: asan_eq <dir> ...     each <dir> holds project.lua and meta.txt ("<buffer length>")
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "termdaw_amd.h"

extern size_t g_eq_launches[3], g_eq_vertices, g_eq_fresh, g_eq_carried;
extern double g_fx_path_gain;

static std::string slurp(const std::string& p) {
    std::string s; FILE* f = fopen(p.c_str(), "rb"); if (!f) return s;
    char b[4096]; size_t n; while ((n = fread(b, 1, sizeof b, f)) > 0) s.append(b, n); fclose(f); return s;
}
int main(int argc, char** argv) {
    size_t renders = 0, rejected = 0, failed = 0, pulls = 0;
    auto bad = [&](const std::string& what) { ++failed; fprintf(stderr, "%s: %s\n", what.c_str(), td_last_error()); };
    for (int a = 1; a < argc; ++a) {
        const std::string dir = argv[a];
        const std::string lua = slurp(dir + "/project.lua");
        const size_t bl = (size_t)atol(slurp(dir + "/meta.txt").c_str());
        if (lua.empty() || !bl) { fprintf(stderr, "bad project dir %s\n", dir.c_str()); return 2; }
        for (int mode = 0; mode < 6; ++mode)
            for (int chunked = 0; chunked < 2; ++chunked) {
                td_state* s = td_state_new(dir.c_str(), 48000, bl);
                if (!s) return 3;
                td_state_set_option(s, "band_mode", mode % 3);
                td_state_set_option(s, "sine_mode", mode < 3 ? 1 : 2);
                if (chunked) td_state_set_option(s, "max_chunk_frames", 4096);
                if (mode % 3 == 2 && chunked) td_state_set_option(s, "band_guard_ppb", 0);   // (every audited render is done again)
                if (!td_state_refresh_source(s, lua.c_str())) { ++rejected; td_state_free(s); continue; }
                td_graph* g = td_state_graph(s);
                const size_t cs = td_state_chunk_count(s);
                std::vector<unsigned char> pcm(td_state_render_to_memory(s, nullptr, 0) + 16);
                if (mode == 5 && !chunked) {
                    td_graph_set_profiling(g, 1);
                    g_fx_path_gain = 0.0;
                }
                for (int k = 0; k < 3; ++k) {
                    if (k == 1 && !td_state_scan_exact(s)) bad(dir + " scan");
                    if (pcm.size() > 16 && !td_state_render_to_memory(s, pcm.data(), pcm.size())) bad(dir + " render");
                    ++renders;
                    if (mode == 5 && !chunked && k == 0) {
                        const char* names[64]; float ms[64]; size_t cnt[64];
                        const size_t n = td_graph_last_kernel_times(g, names, ms, cnt, 64);
                        printf("launches %s:", dir.c_str());
                        for (size_t i = 0; i < n && i < 64; ++i) printf(" %s=%zu", names[i], cnt[i]);
                        printf("\n");
                        printf("guard %s: path=%.9g\n", dir.c_str(), g_fx_path_gain);
                        td_graph_set_profiling(g, 0);
                    }
                }
                if (cs && (mode == 0 || mode == 5)) {
                    // block pulls continue from the carried state; a set_time in between restarts it; then a whole render again
                    std::vector<float> l(bl), r(bl);
                    for (int k = 0; k < 3; ++k) {
                        if (k == 2) { td_graph_set_time(g, 0); td_flowwbank_set_time(td_state_flowwbank(s), 0); }
                        if (td_graph_render_block(g, td_state_samplebank(s), td_state_flowwbank(s), l.data(), r.data()) < 0) bad(dir + " pull");
                        ++pulls;
                    }
                    td_graph_set_time(g, 0);
                    td_flowwbank_set_time(td_state_flowwbank(s), 0);
                    td_graph_reset_normalize_vertices(g);
                    if (!td_graph_render_all(g, td_state_samplebank(s), td_state_flowwbank(s), cs, 24)) bad(dir + " render_all");
                    ++renders;
                    // a batch: this project and a second State of it, merged launches
                    td_state* s2 = td_state_new(dir.c_str(), 48000, bl);
                    if (chunked) td_state_set_option(s2, "max_chunk_frames", 4096);
                    if (s2 && td_state_refresh_source(s2, lua.c_str())) {
                        td_batch* b = td_batch_new();
                        if (td_batch_add(b, g, td_state_samplebank(s), td_state_flowwbank(s)) < 0) bad(dir + " batch add");
                        if (td_batch_add(b, td_state_graph(s2), td_state_samplebank(s2), td_state_flowwbank(s2)) < 0) bad(dir + " batch add");
                        if (!td_batch_render_all(b, cs, 16)) bad(dir + " batch render");
                        if (!td_batch_sync(b)) bad(dir + " batch sync");
                        ++renders;
                        td_batch_free(b);
                    } else {
                        bad(dir + " second state");
                    }
                    if (s2) td_state_free(s2);
                }
                td_state_free(s);
            }
    }
    for (int i = 1; i < 3; ++i)
        if (g_eq_launches[i] != g_eq_launches[0]) { ++failed; fprintf(stderr, "launch counts differ: %zu vs %zu (step %d)\n", g_eq_launches[0], g_eq_launches[i], i); }
    printf("asan_eq done: %d projects, %zu renders, %zu pulls, %zu rejected refreshes, %zu failed calls; k_eq launches %zu "
           "(%zu vertices, %zu entered fresh, %zu entered with carried state)\n",
           argc - 1, renders, pulls, rejected, failed, g_eq_launches[0], g_eq_vertices, g_eq_fresh, g_eq_carried);
    return failed ? 1 : 0;
}
