set_length(20.0);
set_render_samplerate(48000);
set_render_bitdepth(16);
set_output_file("chain.wav");

load_sample("hat", "/nonexistent/fixtures/hat.wav", "");

load_midi_floww("hats", "/nonexistent/fixtures/hats.mid");
load_midi_floww("keys", "/nonexistent/fixtures/keys.mid");
load_lv2("phaser", "http://example.org/plugins/Phaser");

add_sample_lerp("hat", 0.6, 30.0, "hat", "hats", -1, 8);

short = { 0.005, 0.04, 0.0, 0.0, 0.0, 0.0 }
long = { 0.05, 0.2, 0.7, 3.0, 0.3, 0.6 };
add_synth("keys", 0.5, 0.0, "keys", 0.3, 0.4, short, 0.8, 0.6, long, 0.0, {});
add_adsr("gate", 1.0, 0.0, 1.0, "hats", true, true, -1, { 0.02, 0.2, 0.5, 0.3, 0.1, 0.05 });

add_lv2fx("phase", 1.0, 0.0, 0.6, "phaser");

add_normalize("bus", 1.0, 0.0);

connect("hat", "gate");
connect("gate", "bus");
connect("keys", "phase");
connect("phase", "bus");

set_output("bus");
