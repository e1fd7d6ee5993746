-- A looping sample through a nine-value envelope built from variables, beside a triggered one.
set_length(8.0);
set_render_samplerate(48000);
set_render_bitdepth(16);
set_output_file("env.wav");

load_sample("drone", "/nonexistent/fixtures/drone.wav", "");
load_sample("rim", "/nonexistent/fixtures/rim.wav", "");

load_midi_floww("gate", "/nonexistent/fixtures/gate.mid");

add_sample_lerp("rim", 0.8, 10.0, "rim", "gate", -1, 16);
add_sampleloop("drone", 1.0, -10.0, "drone");
low = 0.25;
shape = { 1.0, 0.02, low, 0.1, low, 0.0, 0.0, 0.1, 1.0 };
add_adsr("duck", 1.0, 0.0, 1.0, "gate", false, false, -1, shape);
add_normalize("out", 1.0, 0.0);

connect("rim", "out");
connect("drone", "duck");
connect("duck", "out");

set_output("out");
