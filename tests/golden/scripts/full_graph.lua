-- Every call of the project vocabulary once: samples, MIDI flowws, LV2 plug-ins with parameters, a resource,
-- sample-lerp / synth / sampsyn / lv2fx / band-pass vertices into one normalize.  Asset paths do not exist.
set_length(12.5);
set_render_samplerate(44100);
set_render_bitdepth(24);
set_output_file("mix.wav");

load_sample("clap", "/nonexistent/fixtures/clap.wav", "");
load_sample("tom", "/nonexistent/fixtures/tom-low.wav", "");
load_sample("shaker", "/nonexistent/fixtures/shaker.wav", "");

load_midi_floww("toms", "/nonexistent/fixtures/toms.mid");
load_midi_floww("claps", "/nonexistent/fixtures/claps.mid");
load_midi_floww("lead", "/nonexistent/fixtures/lead.mid");
load_midi_floww("pads", "/nonexistent/fixtures/pads.mid");

load_lv2("delay", "http://example.org/plugins/Delay");
load_lv2("limiter", "http://example.org/plugins/Limiter");

parameter("delay", "Time", 250.0);
parameter("limiter", "Threshold", -3.0);

load_resource("padtable", "/nonexistent/fixtures/pad.wtable");

add_sample_lerp("tom", 1.5, -30.0, "tom", "toms", -1, 32);
add_sample_lerp("clap", 0.7, 15.0, "clap", "claps", 60, 24);
add_sampleloop("shaker", 0.2, 45.0, "shaker");

pluck = { 0.002, 0.05, 0.0, 0.0, 0.0, 0.0 };
swell = { 0.2, 0.3, 0.6, 2.0, 0.4, 0.8 };
add_synth("lead", 0.4, 0.0, "lead", 0.6, 0.1, pluck, 0.9, 0.5, swell, 0.0, {});
--add_synth("unused", 0.5, 0.0, "lead", 0.5, 0.2, pluck, 1.0, 0.7, swell, 0.0, {});
add_sampsyn("pad", 0.3, 0.0, "pads", swell, "padtable");

add_lv2fx("echo", 1.0, 0.0, 0.5, "delay");
add_lv2fx("limit", 1.0, 0.0, 1.0, "limiter");
add_bandpass("hp", 1.0, 0.0, 1.0, 200, 0, true);
add_bandpass("lp", 0.8, 0.0, 0.7, 0, 8000, false)

add_normalize("master", 0.9, 0.0);

connect("tom", "hp");
connect("clap", "echo");
connect("shaker", "lp");
connect("lead", "echo");
connect("pad", "lp");
connect("echo", "limit");
connect("hp", "limit");
connect("lp", "master");
connect("limit", "master");

set_output("master");
