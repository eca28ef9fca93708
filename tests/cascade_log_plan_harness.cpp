// Command-line driver of csrc/cascade_log_plan.hpp (tests/test_cascade_log_plan.py): the cascade log's descriptor check, layout, schedule,
// read descriptors and status word, compiled with the host compiler only.  Tokens, left to right:
//   batch:B                                             the cascade's batch (default 67)
//   desc:capacity:every:first:mask:thrust:ref:err:status   the descriptor
//   check                                               -> "check rc=0 nsel= state= thrust= ref= errs= status= total="  or  "check rc=-1 err=<text>"
//   start                                               check, then CasLogPlan::start (prints like check)
//   stop                                                CasLogPlan::stop
//   tick:n                                              n low-level ticks -> "tick i= slot= missed=" each
//   info                                                -> "info on= records= ticks= missed="
//   read:channel:rec0:nrec:b0:nb                        -> "read rc=0 channel= n= elem= offset= pitch= width= rows= bytes="  or  "read rc=-1 err=<text>"
//   word:ll_status:ll_qp_iter:g_status:g_qp_iter        -> "word value="
#include "cascade_log_plan.hpp"

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
    int B = 67;
    CasLogDesc d = {};
    CasLogPlan plan;
    long long i = 0;
    for (int k = 1; k < argc; k++) {
        const std::vector<std::string> w = split(argv[k]);
        auto num = [&](size_t j) { return j < w.size() ? std::strtoll(w[j].c_str(), nullptr, 0) : 0ll; };
        if (w[0] == "batch") B = (int)num(1);
        else if (w[0] == "desc") {
            d = CasLogDesc{};
            d.capacity = (int)num(1); d.every = (int)num(2); d.first = (int)num(3); d.state_mask = (unsigned)num(4);
            d.record_thrust = (int)num(5); d.record_ref = (int)num(6); d.record_err = (int)num(7); d.record_status = (int)num(8);
        } else if (w[0] == "check" || w[0] == "start") {
            CasLogLayout l = {};
            const char *why = check_cas_log_desc(d, B, &l);
            if (why) std::printf("%s rc=-1 err=%s\n", w[0].c_str(), why);
            else {
                std::printf("%s rc=0 nsel=%d state=%lld thrust=%lld ref=%lld errs=%lld status=%lld total=%lld\n", w[0].c_str(), l.nsel, l.state_bytes,
                            l.thrust_bytes, l.ref_bytes, l.err_bytes, l.status_bytes, l.total());
                if (w[0] == "start") { plan.start(d, l); i = 0; }
            }
        } else if (w[0] == "stop") plan.stop();
        else if (w[0] == "tick") {
            for (long long n = num(1); n > 0; n--) {
                const LogTick t = plan.on_tick();
                std::printf("tick i=%lld slot=%d missed=%d\n", i++, t.slot, (int)t.missed);
            }
        } else if (w[0] == "info")
            std::printf("info on=%d records=%d ticks=%lld missed=%lld\n", (int)plan.on(), plan.records(), plan.ticks(), plan.missed());
        else if (w[0] == "read") {
            CasLogCopy c = {};
            const char *why = plan.read_desc(w.size() > 1 ? w[1].c_str() : nullptr, num(2), num(3), num(4), num(5), &c);
            if (why) std::printf("read rc=-1 err=%s\n", why);
            else
                std::printf("read rc=0 channel=%d n=%d elem=%d offset=%lld pitch=%lld width=%lld rows=%lld bytes=%lld\n", (int)c.channel, c.n, c.elem,
                            c.offset, c.pitch, c.width, c.rows, c.bytes());
        } else if (w[0] == "word")
            std::printf("word value=%d\n", cas_log_status_word((int)num(1), (int)num(2), (int)num(3), (int)num(4)));
        else { std::printf("bad token %s\n", argv[k]); return 2; }
    }
    return 0;
}
