// Host harness of a network slot's host side: what the setters refuse (check_net_desc, check_net_frame, check_net_rivals, check_value_desc: one bad
// description per refusal, each edge of a range, code and message), and for accepted descriptions the record the kernels are handed (net_record,
// value_record: every field written out), net_param_count and the TrainNet that train_net makes of it.  No handle, no device.  One line per case;
// tests/test_net_slot_host.py compares the output with tests/net_slot_check.txt line for line.
// Build: hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -std=c++17 -x hip tools/net_slot_check.cpp -o /tmp/net_slot_check -ldl
#include "../ft_grandprix_amd/csrc/ftgp_api.hip"

// the checks of a policy's description on a handle of R rays, in the setter's order
static int policy_checks(int R, const FtgpNetDesc& d, const FtgpNetFrame* f, const FtgpNetRivals* r)
{
    if (int rc = check_net_desc(R, (int)((double)R / 8.0), d)) return rc;
    if (f) if (int rc = check_net_frame(d, *f)) return rc;
    if (r) if (int rc = check_net_rivals(d, f, *r)) return rc;
    return 0;
}

static void refused(const char* label, int rc)
{
    printf("refused %s: %d %s\n", label, rc, rc ? ftgp_last_error() : "ACCEPTED");
}

// 1080 rays, window [135, 945): beams of 4 rays, 34 .. 235 inside
static FtgpNetDesc good_desc()
{
    FtgpNetDesc d{};
    d.pool = 4; d.max_range = 10.0f; d.beam_first = 40; d.n_beams = 100; d.use_state = 1; d.n_layers = 3;
    d.width[0] = 64; d.width[1] = 64; d.width[2] = 2;
    d.hidden_act = FTGP_ACT_TANH; d.out_act = FTGP_ACT_TANH;
    d.out_scale[0] = d.out_scale[1] = 1.0f;
    return d;
}
static FtgpValueDesc good_value()
{
    FtgpValueDesc d{};
    d.n_layers = 3; d.width[0] = 64; d.width[1] = 64; d.width[2] = 1;
    d.hidden_act = FTGP_ACT_TANH; d.out_act = FTGP_ACT_IDENTITY; d.out_scale = 1.0f;
    return d;
}

template <class Edit> static void bad_desc(const char* label, Edit edit, const FtgpNetFrame* f = nullptr, const FtgpNetRivals* r = nullptr)
{
    FtgpNetDesc d = good_desc();
    edit(d);
    refused(label, policy_checks(1080, d, f, r));
}
template <class Edit> static void bad_frame(const char* label, Edit edit)
{
    FtgpNetFrame f{ 1, 8, 2, 0 };
    edit(f);
    refused(label, policy_checks(1080, good_desc(), &f, nullptr));
}
template <class Edit> static void bad_rivals(const char* label, Edit edit)
{
    FtgpNetFrame f{ 1, 8, 2, 0 };
    FtgpNetRivals r{ 1, 3, { 0, 0 } };
    edit(r);
    refused(label, policy_checks(1080, good_desc(), &f, &r));
}
template <class Edit> static void bad_value(const char* label, Edit edit)
{
    FtgpValueDesc d = good_value();
    edit(d);
    refused(label, check_value_desc(d));
}

static void refusals()
{
    const float inf = INFINITY, nan = NAN;
    refused("nothing wrong", policy_checks(1080, good_desc(), nullptr, nullptr));
    bad_desc("reserved 1", [](FtgpNetDesc& d) { d.reserved = 1; });
    bad_desc("reserved -1", [](FtgpNetDesc& d) { d.reserved = -1; });
    bad_desc("pool 0", [](FtgpNetDesc& d) { d.pool = 0; });
    bad_desc("pool -1", [](FtgpNetDesc& d) { d.pool = -1; });
    bad_desc("pool 7 of 1080", [](FtgpNetDesc& d) { d.pool = 7; });
    bad_desc("max_range 0", [](FtgpNetDesc& d) { d.max_range = 0.0f; });
    bad_desc("max_range -1", [](FtgpNetDesc& d) { d.max_range = -1.0f; });
    bad_desc("max_range inf", [&](FtgpNetDesc& d) { d.max_range = inf; });
    bad_desc("max_range nan", [&](FtgpNetDesc& d) { d.max_range = nan; });
    bad_desc("n_beams 0", [](FtgpNetDesc& d) { d.n_beams = 0; });
    bad_desc("beam_first -1", [](FtgpNetDesc& d) { d.beam_first = -1; });
    bad_desc("n_beams 257", [](FtgpNetDesc& d) { d.pool = 1; d.beam_first = 135; d.n_beams = FTGP_NET_MAX_INPUTS + 1; });
    bad_desc("beam_first 1081", [](FtgpNetDesc& d) { d.beam_first = 1081; });
    bad_desc("window low, pool 1", [](FtgpNetDesc& d) { d.pool = 1; d.beam_first = 134; });
    bad_desc("window low, pool 4", [](FtgpNetDesc& d) { d.beam_first = 33; });
    bad_desc("window high, pool 1", [](FtgpNetDesc& d) { d.pool = 1; d.beam_first = 846; });
    bad_desc("window high, pool 4", [](FtgpNetDesc& d) { d.beam_first = 137; });
    bad_desc("use_state 2", [](FtgpNetDesc& d) { d.use_state = 2; });
    bad_desc("use_state -1", [](FtgpNetDesc& d) { d.use_state = -1; });
    bad_desc("n_layers 0", [](FtgpNetDesc& d) { d.n_layers = 0; });
    bad_desc("n_layers 5", [](FtgpNetDesc& d) { d.n_layers = FTGP_NET_MAX_LAYERS + 1; });
    bad_desc("width behind the last layer", [](FtgpNetDesc& d) { d.width[3] = 1; });
    bad_desc("last width 1", [](FtgpNetDesc& d) { d.width[2] = 1; });
    bad_desc("last width 3", [](FtgpNetDesc& d) { d.width[2] = 3; });
    bad_desc("hidden width 0", [](FtgpNetDesc& d) { d.width[0] = 0; });
    bad_desc("hidden width 129", [](FtgpNetDesc& d) { d.width[1] = FTGP_NET_MAX_HIDDEN + 1; });
    bad_desc("hidden_act -1", [](FtgpNetDesc& d) { d.hidden_act = -1; });
    bad_desc("hidden_act 3", [](FtgpNetDesc& d) { d.hidden_act = 3; });
    bad_desc("out_act -1", [](FtgpNetDesc& d) { d.out_act = -1; });
    bad_desc("out_act 3", [](FtgpNetDesc& d) { d.out_act = 3; });
    for (int k = 0; k < 2; ++k) {
        char label[64];
        snprintf(label, sizeof label, "out_scale[%d] inf", k);  bad_desc(label, [&](FtgpNetDesc& d) { d.out_scale[k] = inf; });
        snprintf(label, sizeof label, "out_scale[%d] nan", k);  bad_desc(label, [&](FtgpNetDesc& d) { d.out_scale[k] = nan; });
        snprintf(label, sizeof label, "out_offset[%d] -inf", k); bad_desc(label, [&](FtgpNetDesc& d) { d.out_offset[k] = -inf; });
        snprintf(label, sizeof label, "out_offset[%d] nan", k); bad_desc(label, [&](FtgpNetDesc& d) { d.out_offset[k] = nan; });
    }
    // n_in one above FTGP_NET_MAX_INPUTS by each of its three routes (pool 1: 256 beams fit the window)
    const FtgpNetFrame most_f{ 1, FTGP_MAX_LOOKAHEAD, 3, 0 };
    const FtgpNetRivals most_r{ 1, FTGP_MAX_RIVALS, { 0, 0 } };
    const int over = FTGP_NET_MAX_INPUTS + 1 - FTGP_NET_STATE_INPUTS;
    bad_desc("n_in 257 by the state inputs", [&](FtgpNetDesc& d) { d.pool = 1; d.beam_first = 135; d.n_beams = over; });
    bad_desc("n_in 257 by the frame inputs", [&](FtgpNetDesc& d) { d.pool = 1; d.beam_first = 135; d.n_beams = over - ftgp_net_frame_inputs(&most_f); }, &most_f);
    bad_desc("n_in 257 by the rival inputs", [&](FtgpNetDesc& d) { d.pool = 1; d.beam_first = 135; d.n_beams = over - ftgp_net_frame_inputs(&most_f) - ftgp_net_rival_inputs(&most_r); },
             &most_f, &most_r);
    // wrong in two ways: the first check in the setter's order names the call
    bad_desc("n_layers 0 and n_in 257", [&](FtgpNetDesc& d) { d.pool = 1; d.beam_first = 135; d.n_beams = over; d.n_layers = 0; });
    bad_desc("n_in 257 and hidden width 0", [&](FtgpNetDesc& d) { d.pool = 1; d.beam_first = 135; d.n_beams = over; d.width[0] = 0; });
    bad_desc("hidden_act 3 and out_scale[0] nan", [&](FtgpNetDesc& d) { d.hidden_act = 3; d.out_scale[0] = nan; });
    bad_desc("use_state 2 and n_layers 5", [](FtgpNetDesc& d) { d.use_state = 2; d.n_layers = 5; });
    bad_frame("frame: nothing wrong", [](FtgpNetFrame&) {});
    bad_frame("frame: enabled 2", [](FtgpNetFrame& f) { f.enabled = 2; });
    bad_frame("frame: enabled -1", [](FtgpNetFrame& f) { f.enabled = -1; });
    bad_frame("frame: n_ahead -1", [](FtgpNetFrame& f) { f.n_ahead = -1; });
    bad_frame("frame: n_ahead 17", [](FtgpNetFrame& f) { f.n_ahead = FTGP_MAX_LOOKAHEAD + 1; });
    bad_frame("frame: n_ahead 17 while off", [](FtgpNetFrame& f) { f.enabled = 0; f.n_ahead = FTGP_MAX_LOOKAHEAD + 1; });
    bad_frame("frame: stride 0", [](FtgpNetFrame& f) { f.stride = 0; });
    bad_frame("frame: stride 51", [](FtgpNetFrame& f) { f.stride = 51; });
    bad_frame("frame: reserved 1", [](FtgpNetFrame& f) { f.reserved = 1; });
    bad_rivals("rivals: nothing wrong", [](FtgpNetRivals&) {});
    bad_rivals("rivals: enabled 2", [](FtgpNetRivals& r) { r.enabled = 2; });
    bad_rivals("rivals: enabled -1", [](FtgpNetRivals& r) { r.enabled = -1; });
    bad_rivals("rivals: n_rivals -1", [](FtgpNetRivals& r) { r.n_rivals = -1; });
    bad_rivals("rivals: n_rivals 8", [](FtgpNetRivals& r) { r.n_rivals = FTGP_MAX_RIVALS + 1; });
    bad_rivals("rivals: n_rivals 8 while off", [](FtgpNetRivals& r) { r.enabled = 0; r.n_rivals = FTGP_MAX_RIVALS + 1; });
    bad_rivals("rivals: reserved[0] 1", [](FtgpNetRivals& r) { r.reserved[0] = 1; });
    bad_rivals("rivals: reserved[1] 1", [](FtgpNetRivals& r) { r.reserved[1] = 1; });
    bad_value("value: nothing wrong", [](FtgpValueDesc&) {});
    bad_value("value: reserved 1", [](FtgpValueDesc& d) { d.reserved = 1; });
    bad_value("value: n_layers 0", [](FtgpValueDesc& d) { d.n_layers = 0; });
    bad_value("value: n_layers 5", [](FtgpValueDesc& d) { d.n_layers = FTGP_NET_MAX_LAYERS + 1; });
    bad_value("value: width behind the last layer", [](FtgpValueDesc& d) { d.width[3] = 1; });
    bad_value("value: last width 0", [](FtgpValueDesc& d) { d.width[2] = 0; });
    bad_value("value: last width 2", [](FtgpValueDesc& d) { d.width[2] = 2; });
    bad_value("value: hidden width 0", [](FtgpValueDesc& d) { d.width[0] = 0; });
    bad_value("value: hidden width 129", [](FtgpValueDesc& d) { d.width[1] = FTGP_NET_MAX_HIDDEN + 1; });
    bad_value("value: hidden_act -1", [](FtgpValueDesc& d) { d.hidden_act = -1; });
    bad_value("value: hidden_act 3", [](FtgpValueDesc& d) { d.hidden_act = 3; });
    bad_value("value: out_act -1", [](FtgpValueDesc& d) { d.out_act = -1; });
    bad_value("value: out_act 3", [](FtgpValueDesc& d) { d.out_act = 3; });
    bad_value("value: out_scale inf", [&](FtgpValueDesc& d) { d.out_scale = inf; });
    bad_value("value: out_scale nan", [&](FtgpValueDesc& d) { d.out_scale = nan; });
    bad_value("value: out_offset -inf", [&](FtgpValueDesc& d) { d.out_offset = -inf; });
    bad_value("value: out_offset nan", [&](FtgpValueDesc& d) { d.out_offset = nan; });
    bad_value("value: reserved 1 and n_layers 0", [](FtgpValueDesc& d) { d.reserved = 1; d.n_layers = 0; });
    bad_value("value: out_act 3 and out_scale nan", [&](FtgpValueDesc& d) { d.out_act = 3; d.out_scale = nan; });
}

// every field of a record, one by one (padding is not specified: no raw bytes), the parameter count and the TrainNet with gradient offset g_off
static void print_record(const NetDev& N, int g_off)
{
    printf(" | N %d %d %d %d %d %d %d %d w", N.defined, N.pool, N.beam_first, N.n_beams, N.use_state, N.n_layers, N.hidden_act, N.out_act);
    for (int l = 0; l <= FTGP_NET_MAX_LAYERS; ++l) printf(" %d", N.width[l]);
    printf(" wo");
    for (int l = 0; l < FTGP_NET_MAX_LAYERS; ++l) printf(" %d", N.w_off[l]);
    printf(" bo");
    for (int l = 0; l < FTGP_NET_MAX_LAYERS; ++l) printf(" %d", N.b_off[l]);
    printf(" nf %d fr %d %d M %a %a os %a %a oo %a %a p %d rv %d %d em %d", N.n_floats, N.frame_first, N.frame_shape, (double)N.max_range, (double)N.inv_max_range,
           (double)N.out_scale[0], (double)N.out_scale[1], (double)N.out_offset[0], (double)N.out_offset[1], N.params != nullptr, N.rival_first, N.rival_shape, N.env_member != nullptr);
    printf(" | count %zu", net_param_count(N));
    static const float anchor = 0.0f;
    const TrainNet t = train_net(N, &anchor, g_off);
    printf(" | T %d %d %d %d w", t.n_layers, t.hidden_act, t.out_act, t.n_floats);
    for (int l = 0; l <= FTGP_NET_MAX_LAYERS; ++l) printf(" %d", t.width[l]);
    printf(" wo");
    for (int l = 0; l < FTGP_NET_MAX_LAYERS; ++l) printf(" %d", t.w_off[l]);
    printf(" bo");
    for (int l = 0; l < FTGP_NET_MAX_LAYERS; ++l) printf(" %d", t.b_off[l]);
    printf(" xo");
    for (int l = 0; l <= FTGP_NET_MAX_LAYERS; ++l) printf(" %d", t.x_off[l]);
    printf(" os %a %a oo %a %a p %d g %d %d\n", (double)t.out_scale[0], (double)t.out_scale[1], (double)t.out_offset[0], (double)t.out_offset[1], t.params == &anchor, t.g_off, t.pad);
}

// one accepted policy and the value net of the same layers on its input width
static void accepted(int R, int layers, int hidden, int use_state, const FtgpNetFrame* f, const FtgpNetRivals* r)
{
    FtgpNetDesc d{};
    // beams inside the window [R / 8, R - R / 8): 36 rays: 28 of 1 ray; 64: 24 of 2; 1080: 100 of 4
    d.pool = R == 36 ? 1 : R == 64 ? 2 : 4; d.beam_first = R == 1080 ? 34 : 4; d.n_beams = R == 36 ? 28 : R == 64 ? 24 : 100;
    d.max_range = R == 36 ? 3.0f : 10.0f;
    d.use_state = use_state; d.n_layers = layers;
    for (int l = 0; l < layers; ++l) d.width[l] = l == layers - 1 ? 2 : hidden;
    d.hidden_act = layers % 2 ? FTGP_ACT_TANH : FTGP_ACT_RELU; d.out_act = use_state ? FTGP_ACT_TANH : FTGP_ACT_IDENTITY;
    d.out_scale[0] = 2.0f; d.out_scale[1] = 0.5f; d.out_offset[0] = 1.5f; d.out_offset[1] = -0.25f;
    char label[160];
    snprintf(label, sizeof label, "rays %d layers %d hidden %d state %d frame %d/%d/%d rivals %d/%d", R, layers, hidden, use_state, f ? f->enabled : -1, f ? f->n_ahead : 0,
             f ? f->stride : 0, r ? r->enabled : -1, r ? r->n_rivals : 0);
    const int rc = policy_checks(R, d, f, r);
    printf("policy %s: %d", label, rc);
    if (rc) { printf(" %s\n", ftgp_last_error()); return; }
    const NetDev N = net_record(d, f, r);
    print_record(N, 0);
    FtgpValueDesc v{};
    v.n_layers = layers;
    for (int l = 0; l < layers; ++l) v.width[l] = l == layers - 1 ? 1 : hidden;
    v.hidden_act = d.hidden_act; v.out_act = FTGP_ACT_IDENTITY; v.out_scale = 3.0f; v.out_offset = -1.0f;
    const int vrc = check_value_desc(v);
    printf("value %s: %d", label, vrc);
    if (vrc) { printf(" %s\n", ftgp_last_error()); return; }
    print_record(value_record(v, N.width[0]), N.n_floats);
}

int main()
{
    refusals();
    const FtgpNetFrame frames[3] = { { 0, 0, 1, 0 }, { 1, 0, 1, 0 }, { 1, FTGP_MAX_LOOKAHEAD, 3, 0 } };      // off, on with no points, on with the most
    const FtgpNetRivals rivals[3] = { { 0, 0, { 0, 0 } }, { 1, 0, { 0, 0 } }, { 1, FTGP_MAX_RIVALS, { 0, 0 } } };
    const int hidden[5] = { 1, 63, 64, 65, FTGP_NET_MAX_HIDDEN };
    for (int R : { 36, 64, 1080 }) {
        // every layer count and hidden width, state inputs on and off: without the two structs, and with the widest of both
        for (int layers = 1; layers <= FTGP_NET_MAX_LAYERS; ++layers)
            for (int h = 0; h < (layers == 1 ? 1 : 5); ++h)
                for (int use_state = 0; use_state < 2; ++use_state) {
                    accepted(R, layers, layers == 1 ? 0 : hidden[h], use_state, nullptr, nullptr);
                    accepted(R, layers, layers == 1 ? 0 : hidden[h], use_state, &frames[2], &rivals[2]);
                }
        // every pairing of the frame and the rival inputs on one shape
        for (int use_state = 0; use_state < 2; ++use_state)
            for (const FtgpNetFrame& f : frames)
                for (const FtgpNetRivals& r : rivals) accepted(R, 2, 64, use_state, &f, &r);
    }
    return 0;
}
