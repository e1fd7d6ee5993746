// What tests/asan_fx.cpp and the mock of the one effect kind linked beside it (mock_delay.cpp, mock_sat.cpp, mock_chorus.cpp,
// mock_reverb.cpp) share: the mock's counters under one set of names, and what the driver has to know about the kind.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include <vector>

struct td_state;

// ---- tests/mock_guard.cpp: the listeners at the guard's launches
extern double g_fx_path_gain;   // the last guarded launch's static gain to the output (0: none since the driver cleared it)
extern int g_fx_force_redo;     // every audited render is to be done again

// ---- the mock's
extern size_t g_fx_launches[3];   // per launch of the kind, in the order of FxHooks::closing's words
extern size_t g_fx_vertices, g_fx_single, g_fx_fresh, g_fx_carried;
extern int g_fx_after_set_time;   // the driver has called td_graph_set_time and not submitted since: every vertex must enter with nothing of its line
extern size_t g_fx_restarts;      // descriptors checked under that flag
extern size_t g_fx_short;         // descriptors whose chunk was shorter than the line
extern std::vector<double> g_fx_entry_log;   // per descriptor that enters with its line: the stamp found there

struct FxHooks {
    const char* name;                                         // the driver is asan_<name>
    void (*options)(td_state* s, int mode, int chunked);      // the kind's debug.* options of a mode (0 .. 5) and chunking
    bool (*closing)();                                        // the launch counts' invariant at the end (false: violated, and said on stderr)
    void (*summary)();                                        // the summary line's words behind "... failed calls; "
};
extern const FxHooks g_fx;
