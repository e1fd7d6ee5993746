// Sanitizer run of the mastering host side on random projects (built by tests/test_master_host.py with g++
// -fsanitize=address,undefined against tests/mock_hip.cpp + tests/mock_stems.cpp + tests/mock_master.cpp -- no GPU, nothing
// computed): every project renders through its State with mastering on and its stems set, at 16 and 24 bits and resampled at
// 8 bits; its graph is mastered again with td_graph_master at other targets and windows; bad parameters and a graph with no
// render fail; then -- stems cleared -- a batch of the project is mastered with td_batch_master, and td_master_f32 runs on frames.
//   usage: asan_master <dir> ...     each <dir> holds project.lua, meta.txt ("<buffer length>") and stems.txt (one name per line)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "termdaw_amd.h"

extern size_t g_loud_launches, g_master_launches[4], g_master_signals;

static std::string slurp(const std::string& p) {
    std::string s; FILE* f = fopen(p.c_str(), "rb"); if (!f) return s;
    char b[4096]; size_t n; while ((n = fread(b, 1, sizeof b, f)) > 0) s.append(b, n); fclose(f); return s;
}
int main(int argc, char** argv) {
    size_t mastered = 0, rejected = 0, failed = 0, short_ = 0;
    // a call that succeeded; one that failed because the project is too short to measure (fewer than 4 hops) is counted apart
    auto done = [&](int r, const std::string& what) {
        if (r) { ++mastered; return true; }
        if (strstr(td_last_error(), "nothing to master")) { ++short_; return false; }
        ++failed;
        fprintf(stderr, "%s: %s\n", what.c_str(), td_last_error());
        return false;
    };
    double out[TD_MASTER_FIELDS * 2];
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
        if (td_graph_master(g, -14.0, -1.0, 5.0, 100.0, out) || !strstr(td_last_error(), "no whole render")) ++failed;
        if (td_state_set_master(s, 1, -61.0, -1.0) || !strstr(td_last_error(), "target_lufs")) ++failed;
        if (!td_state_set_master(s, 1, -16.0, -1.0)) ++failed;
        if (!td_state_set_stems(s, names.data(), names.size())) ++failed;
        const size_t cs = td_state_chunk_count(s);
        std::vector<unsigned char> pcm(td_state_render_to_memory(s, nullptr, 0) + 8);
        for (int k = 0; k < 2 && cs; ++k) {
            if (k == 1 && !td_state_set_master(s, 1, -23.0, -2.0)) ++failed;
            if (!done(td_state_render_to_memory(s, pcm.data(), pcm.size()) != 0, dir)) continue;
            if (!td_state_master_report(s, out) || out[13] < 1.0 || out[13] > 5.0 || out[12] != 1.0) ++failed;
        }
        if (cs) {
            const size_t n = td_graph_render_all(g, td_state_samplebank(s), td_state_flowwbank(s), cs, 24);
            if (!n) ++failed;
            td_graph_set_time(g, 0);
            td_flowwbank_set_time(td_state_flowwbank(s), 0);
            td_graph_reset_normalize_vertices(g);
            const double looks[3] = {0.1, 5.0, 100.0};
            for (double la : looks) (void)done(td_graph_master(g, -14.0, -1.0, la, 50.0, out), dir);
            if (td_graph_master(g, -14.0, 0.5, 5.0, 100.0, out) || !strstr(td_last_error(), "ceiling_dbtp")) ++failed;
            if (td_graph_master(g, -14.0, -1.0, 0.05, 100.0, out) || !strstr(td_last_error(), "lookahead_ms")) ++failed;
            if (td_graph_master(g, -14.0, -1.0, 5.0, 0.5, out) || !strstr(td_last_error(), "release_ms")) ++failed;
            const size_t r = td_graph_render_all_resampled(g, td_state_samplebank(s), td_state_flowwbank(s), cs, 8, 48000, 44100);
            if (!r) ++failed;
            td_graph_set_time(g, 0);
            td_flowwbank_set_time(td_state_flowwbank(s), 0);
            td_graph_reset_normalize_vertices(g);
            if (done(td_graph_master(g, -20.0, -3.0, 5.0, 100.0, out), dir) && (out[7] != 44100.0 || out[6] != (double)r)) ++failed;
            // a batch of the project (stems cleared: batches refuse them)
            if (!td_state_set_stems(s, nullptr, 0)) ++failed;
            td_batch* b = td_batch_new();
            if (td_batch_add(b, g, td_state_samplebank(s), td_state_flowwbank(s)) < 0) ++failed;
            if (!td_batch_render_all(b, cs, 16)) ++failed;
            (void)done(td_batch_master(b, -14.0, -1.0, 5.0, 100.0, out), dir);
            td_batch_free(b);
        }
        td_state_free(s);
    }
    {   // host frames
        std::vector<float> x(2 * 48000), y(x.size());
        for (size_t i = 0; i < x.size(); ++i) x[i] = 0.25f * (float)sin(0.05 * (double)i);
        if (done(td_master_f32(x.data(), 48000, 48000, -14.0, -1.0, 5.0, 100.0, y.data(), out), "f32") && y != x) ++failed;   // (the mock apply copies the frames through)
    }
    printf("asan_master done: %d projects, %zu masterings, %zu too short, %zu rejected refreshes, %zu failed calls; k_loudness launches %zu, "
           "k_master launches %zu %zu %zu %zu (%zu signals)\n",
           argc - 1, mastered, short_, rejected, failed, g_loud_launches, g_master_launches[0], g_master_launches[1], g_master_launches[2],
           g_master_launches[3], g_master_signals);
    return failed ? 1 : 0;
}
