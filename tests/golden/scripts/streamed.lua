-- The stream workflow: no length or output settings, events arrive on declared streams.
load_sample("bongo", "/nonexistent/fixtures/bongo.wav", "mix-down");
load_sample("cowbell", "/nonexistent/fixtures/cowbell.wav", "normalize-seperate");

load_resource("organ-table", "/nonexistent/fixtures/organ.wtable");
load_resource("sub-table", "/nonexistent/fixtures/sub.wtable");

declare_stream("bongo");
declare_stream("cowbell");
declare_stream("organ");
declare_stream("sub")

add_sample_lerp("bongo", 1.2, -15.0, "bongo", "bongo", -1, 20);
add_sample_lerp("cowbell", 0.5, 25.0, "cowbell", "cowbell", -1, 20);

organ_adsr = { 0.02, 0.5, 0.9, 4.0, 0.1, 0.3 };
-- name, gain, angle, floww, adsr_conf, resource
add_sampsyn("organ", 0.6, 0.0, "organ", organ_adsr, "organ-table");
add_sampsyn("sub", 1.5, 0.0, "sub", { 0.01, 1.0, 1.0, 2.0, 0.0, 0.1 }, "sub-table");

add_normalize("mix", 0.8, 0.0);

connect("bongo", "mix");
connect("cowbell", "mix");
connect("organ", "mix");
connect("sub", "mix");

set_output("mix");
