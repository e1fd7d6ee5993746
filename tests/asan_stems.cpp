// Sanitizer run of the stems on random projects (built by tests/test_stems_host.py with g++ -fsanitize=address,undefined
// against tests/mock_hip.cpp + tests/mock_stems.cpp -- no GPU, nothing computed): every project goes through the front-end
// and C ABI with its stems set -- fresh, scanned and continued renders, a resampled render, the State's stem files, a block
// pull and a batch that must refuse -- in every band mode with sine modes 1 and 2, un-chunked and in 4 096-frame chunks.  It
// prints what the engine reports it compiled: the fusions the stems switched off (engine option "debug.stem_taps").
//   usage: asan_stems <dir> ...     each <dir> holds project.lua, meta.txt ("<buffer length>") and stems.txt (one name per line)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "termdaw_amd.h"

extern size_t g_stem_launches, g_stem_buffers, g_stem_loops, g_stem_f32;

static std::string slurp(const std::string& p) {
    std::string s; FILE* f = fopen(p.c_str(), "rb"); if (!f) return s;
    char b[4096]; size_t n; while ((n = fread(b, 1, sizeof b, f)) > 0) s.append(b, n); fclose(f); return s;
}
int main(int argc, char** argv) {
    size_t renders = 0, rejected = 0, failed = 0, stem_reads = 0;
    unsigned long taps = 0;   // engine option "debug.stem_taps" over every State: the fusions the stems switched off
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
        for (int mode = 0; mode < 6; ++mode)
            for (int chunked = 0; chunked < 2; ++chunked) {
                td_state* s = td_state_new(dir.c_str(), 48000, bl);
                if (!s) return 3;
                td_state_set_option(s, "band_mode", mode % 3);
                td_state_set_option(s, "sine_mode", mode < 3 ? 1 : 2);
                if (chunked) td_state_set_option(s, "max_chunk_frames", 4096);
                if (mode % 3 == 2 && chunked) td_state_set_option(s, "band_guard_ppb", 0);   // (every audited render is done again)
                if (!td_state_refresh_source(s, lua.c_str())) { ++rejected; td_state_free(s); continue; }
                if (!td_state_set_stems(s, names.data(), names.size())) ++failed;
                td_graph* g = td_state_graph(s);
                std::vector<unsigned char> pcm(td_state_render_to_memory(s, nullptr, 0) + 16);
                for (int k = 0; k < 3; ++k) {
                    if (k == 1 && !td_state_scan_exact(s)) ++failed;
                    if (pcm.size() > 16) {
                        if (!td_state_render_to_memory(s, pcm.data(), pcm.size())) { ++failed; fprintf(stderr, "%s: %s\n", dir.c_str(), td_last_error()); }
                        if (td_graph_stem_count(g) != names.size()) ++failed;
                        for (size_t i = 0; i < names.size(); ++i) {
                            if (!td_graph_read_stem_pcm(g, i, pcm.data(), pcm.size() - 16)) ++failed;
                            (void)td_graph_stem_peak(g, i);
                            ++stem_reads;
                        }
                    }
                    ++renders;
                }
                {
                    long v = 0;
                    if (!td_graph_get_option(g, "debug.stem_taps", &v)) ++failed;
                    taps |= (unsigned long)v;
                }
                if (pcm.size() > 16 && mode == 0) {
                    // the resampled arm, the stem files, a block pull, and a batch that must refuse
                    const size_t cs = td_state_chunk_count(s);
                    if (!td_graph_render_all_resampled(g, td_state_samplebank(s), td_state_flowwbank(s), cs, 24, 48000, 44100)) ++failed;
                    for (size_t i = 0; i < names.size(); ++i) { if (!td_graph_read_stem_pcm(g, i, pcm.data(), 16)) ++failed; ++stem_reads; }
                    ++renders;
                    if (!td_state_render(s, (dir + "/out.wav").c_str())) { ++failed; fprintf(stderr, "%s: %s\n", dir.c_str(), td_last_error()); }
                    ++renders;
                    std::vector<float> l(bl), r(bl);
                    if (td_graph_render_block(g, td_state_samplebank(s), td_state_flowwbank(s), l.data(), r.data()) < 0) ++failed;
                    if (td_graph_stem_count(g) != names.size()) ++failed;
                    td_batch* b = td_batch_new();
                    if (td_batch_add(b, g, td_state_samplebank(s), td_state_flowwbank(s)) < 0) ++failed;
                    if (td_batch_render_all(b, 2, 16) != 0 || !strstr(td_last_error(), "stems")) ++failed;
                    td_batch_free(b);
                }
                td_state_free(s);
            }
    }
    printf("asan_stems done: %d projects, %zu renders, %zu rejected refreshes, %zu failed calls, %zu stem reads; "
           "k_stems launches %zu (%zu buffer descriptors, %zu loop descriptors, %zu with an f32 copy); stem taps %lu\n",
           argc - 1, renders, rejected, failed, stem_reads, g_stem_launches, g_stem_buffers, g_stem_loops, g_stem_f32, taps);
    return failed ? 1 : 0;
}
