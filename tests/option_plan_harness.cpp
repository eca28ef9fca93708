// Command-line face of csrc/option_plan.hpp (host only: no HIP) for tests/test_option_plan.py.  Tokens, in order:
//   N= nx= nu= K= pairs= bsoft= boxpack=   the handle's sizes and facts for what follows (defaults: N 6, nx 14, nu 2, K 3, pairs 1, bsoft 0, boxpack 1)
//   set:<name>:<value>     parse_option -> "set name=<name> rc=<code> value=<normalised, %.17g> fx=<effects> stored=<what the row's member of a
//                          default Options then holds> err=<text to the end of the line>"; <value> as strtod reads it (nan, inf, -inf, 0x1p53)
//   null:<value>           the same for a null name
//   names                  "name <name>" per row of the table, in its order
//   defaults:<0|1>         "defaults <member>=<value> ..." of Options::defaults(model has pairs)
// fx: the effect bits by name, joined by '|' ("-": none).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "option_plan.hpp"

using namespace usv;

static std::string fx_names(unsigned fx)
{
    static const struct { unsigned bit; const char *name; } NAMES[] = {
        {FX_KEEPS_AHEAD, "keeps_ahead"}, {FX_IF_CHANGED, "if_changed"}, {FX_CAPS, "caps"}, {FX_COND_RELEASE, "cond_release"},
        {FX_MAP_CHANGED, "map_changed"}, {FX_LAYOUT_DIRTY, "layout_dirty"}, {FX_TRACKS_DIRTY, "tracks_dirty"}, {FX_UPLOAD_SPEC, "upload_spec"},
        {FX_HOOK, "hook"}};
    std::string s;
    for (const auto &n : NAMES)
        if (fx & n.bit) { s += s.empty() ? "" : "|"; s += n.name; fx &= ~n.bit; }
    if (fx) s += "|?"; // (a bit without a name here)
    return s.empty() ? "-" : s;
}

static void set(const char *name, const char *shown, double v, const OptFacts &f)
{
    const OptParse p = parse_option(name, v, f);
    std::string stored = "-";
    if (p.rc == 0 && p.row->at.type != OptMember::NONE) {
        Options o;
        store(o, p.row->at, p.value);
        char buf[64];
        std::snprintf(buf, sizeof buf, "%.17g", load(o, p.row->at));
        stored = buf;
    }
    std::printf("set name=%s rc=%d value=%.17g fx=%s stored=%s err=%s\n", shown, p.rc, p.value, p.row ? fx_names(p.row->fx).c_str() : "-",
                stored.c_str(), p.err.c_str());
}

int main(int argc, char **argv)
{
    OptFacts f = {6, 14, 2, 3, true, false, true};
    for (int i = 1; i < argc; i++) {
        const std::string t = argv[i];
        const size_t eq = t.find('='), c1 = t.find(':');
        if (eq != std::string::npos && c1 == std::string::npos) {
            const std::string key = t.substr(0, eq);
            const int v = std::atoi(t.c_str() + eq + 1);
            if (key == "N") f.N = v;
            else if (key == "nx") f.nx = v;
            else if (key == "nu") f.nu = v;
            else if (key == "K") f.K = v;
            else if (key == "pairs") f.has_pairs = v != 0;
            else if (key == "bsoft") f.any_bsoft = v != 0;
            else if (key == "boxpack") f.boxpack_ok = v != 0;
            else { std::fprintf(stderr, "unknown size '%s'\n", key.c_str()); return 2; }
        } else if (t == "names") {
            for (const OptRow &r : OPTION_TABLE) std::printf("name %s\n", r.name);
        } else if (t.rfind("defaults:", 0) == 0) {
            const Options o = Options::defaults(t[9] == '1');
            std::printf("defaults pipeline=%d sort_enabled=%d sort_two=%d max_waves=%ld lin_force=%d lin_pairs=%d aux_lds=%d lds_mode=%d wide_mode=%d "
                        "wide_waves=%d dynamic_rows=%d handover_iter=%d handover_lds=%d handover_co=%d co_spin_limit=%d co_wgs=%ld noise_mask=%u "
                        "instance_offset=%lld merge_rows=%d step_on_advance=%d pf_predict=%d pf_margin=%.17g cond_N2=%d tracks_on=%d\n",
                        o.pipeline, o.sort_enabled, o.sort_two, o.max_waves, o.lin_force, o.lin_pairs, o.aux_lds, o.lds_mode, o.wide_mode, o.wide_waves,
                        o.dynamic_rows, o.handover_iter, o.handover_lds, o.handover_co, o.co_spin_limit, o.co_wgs, o.noise_mask, o.instance_offset,
                        o.merge_rows, o.step_on_advance, o.pf_predict, o.pf_margin, o.cond_N2, o.tracks_on);
        } else if (t.rfind("null:", 0) == 0) {
            set(nullptr, "(null)", std::strtod(t.c_str() + 5, nullptr), f);
        } else if (t.rfind("set:", 0) == 0) {
            const size_t c2 = t.rfind(':');
            if (c2 < 4) { std::fprintf(stderr, "set:<name>:<value>\n"); return 2; }
            const std::string name = t.substr(4, c2 - 4);
            set(name.c_str(), name.c_str(), std::strtod(t.c_str() + c2 + 1, nullptr), f);
        } else { std::fprintf(stderr, "unknown token '%s'\n", t.c_str()); return 2; }
    }
    return 0;
}
