// Command-line driver of csrc/log_plan.hpp (tests/test_log_plan.py): the closed-loop log's descriptor check, layout, schedule and read
// descriptors, compiled with the host compiler only.  Tokens, left to right:
//   dims:nx:nu:B                                   the handle's sizes (default 14:2:70)
//   desc:capacity:every:first:mask:u:status:err_first   the descriptor without error channels
//   err:a:b:c                                      appends an error channel (c: strtod, "nan" and "inf" included)
//   nerr:n                                         overrides n_err
//   check                                          -> "check rc=0 nsel= x= u= status= sums= total="  or  "check rc=-1 err=<text>"
//   start                                          check, then LogPlan::start (prints like check)
//   tick:n                                         n hand-overs -> "tick i= slot= errors= missed=" each
//   info                                           -> "info records= handovers= missed= err_count="
//   read:channel:rec0:nrec:b0:nb                   -> "read rc=0 channel= n= elem= offset= pitch= width= rows= bytes="  or  "read rc=-1 err=<text>"
#include "log_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace usv;

static std::vector<std::string> split(const std::string &s)
{
    std::vector<std::string> out;
    size_t a = 0;
    for (;;) {
        const size_t b = s.find(':', a);
        out.push_back(s.substr(a, b == std::string::npos ? b : b - a));
        if (b == std::string::npos) return out;
        a = b + 1;
    }
}

int main(int argc, char **argv)
{
    int nx = 14, nu = 2, B = 70;
    LogDesc d = {};
    LogPlan plan;
    long long i = 0;
    for (int k = 1; k < argc; k++) {
        const std::vector<std::string> w = split(argv[k]);
        auto num = [&](size_t j) { return j < w.size() ? std::strtoll(w[j].c_str(), nullptr, 0) : 0ll; };
        if (w[0] == "dims") { nx = (int)num(1); nu = (int)num(2); B = (int)num(3); }
        else if (w[0] == "desc") {
            d = LogDesc{};
            d.capacity = (int)num(1); d.every = (int)num(2); d.first = (int)num(3); d.state_mask = (unsigned)num(4);
            d.record_u = (int)num(5); d.record_status = (int)num(6); d.err_first = (int)num(7);
        } else if (w[0] == "err") {
            if (d.n_err >= LOG_ERR_MAX) { std::printf("bad token %s\n", argv[k]); return 2; }
            d.err_a[d.n_err] = (int)num(1); d.err_b[d.n_err] = (int)num(2);
            d.err_c[d.n_err] = w.size() > 3 ? std::strtod(w[3].c_str(), nullptr) : 0.0;
            d.n_err++;
        } else if (w[0] == "nerr") d.n_err = (int)num(1);
        else if (w[0] == "check" || w[0] == "start") {
            LogLayout l = {};
            const char *why = check_log_desc(d, nx, nu, B, &l);
            if (why) std::printf("%s rc=-1 err=%s\n", w[0].c_str(), why);
            else {
                std::printf("%s rc=0 nsel=%d x=%lld u=%lld status=%lld sums=%lld total=%lld\n", w[0].c_str(), l.nsel, l.x_bytes, l.u_bytes,
                            l.status_bytes, l.sums_bytes, l.total());
                if (w[0] == "start") { plan.start(d, l); i = 0; }
            }
        } else if (w[0] == "tick") {
            for (long long n = num(1); n > 0; n--) {
                const LogTick t = plan.on_handover();
                std::printf("tick i=%lld slot=%d errors=%d missed=%d\n", i++, t.slot, (int)t.errors, (int)t.missed);
            }
        } else if (w[0] == "info")
            std::printf("info records=%d handovers=%lld missed=%lld err_count=%lld\n", plan.records, plan.handovers, plan.missed, plan.err_count);
        else if (w[0] == "read") {
            LogCopy c = {};
            const char *why = plan.read_desc(w.size() > 1 ? w[1].c_str() : nullptr, num(2), num(3), num(4), num(5), &c);
            if (why) std::printf("read rc=-1 err=%s\n", why);
            else
                std::printf("read rc=0 channel=%d n=%d elem=%d offset=%lld pitch=%lld width=%lld rows=%lld bytes=%lld\n", (int)c.channel, c.n, c.elem,
                            c.offset, c.pitch, c.width, c.rows, c.bytes());
        } else { std::printf("bad token %s\n", argv[k]); return 2; }
    }
    return 0;
}
