// The caller-visible fields, the arena and the host mirror's bookkeeping (csrc/field_plan.hpp) on the host: a handle made of numbers and
// three byte buffers, driven from the command line.
// Arguments, in order.  name=value sets a size (B N nx nu ny ny_e K nlam exported mirror; before the first operation).  Table queries:
// "row:NAME" prints the row's rights and flags, "q:set|get:NAME:STAGE" what resolve and stage_check say, "layout" the arena.  Operations, each
// doing what usvmpc.hip does around the same HostMirror calls and printing one "op" line (rc, whether the mirror served it, whether the host
// had to wait first) followed by one "copy" line per copy descriptor the mirror emitted (up: flush, now: immediate, back: read-back):
//   set:NAME:STAGE get:NAME:STAGE (STAGE -1: the whole field)   flush   solve (flush, device-side results, read-back; not synchronised)
//   status (usvmpc_solve's read)   advance (flush, device-side x0)   frontend (flush, device-side yref / p)   devptr   ext:NAME:STAGE (a
//   caller's kernel behind a handed-out pointer)   sync   drop (option "host_mirror" 0)
// "model:SEED:OPS" runs OPS random operations of these kinds instead, silently, and prints one summary line.
// The model behind every operation: `dev` stands for the device arena, `mir` for the pinned mirror, and `twin` is the direct path - one buffer
// every set, get and device-side write is applied to at once.  Copies are queued like work on a stream and carried out when the host
// waits or device-side work behind them runs.  Checked throughout (exit code 1 with a message): every get equals the twin's; at every flush
// point the device arena equals the twin; the host touches the mirror only while no copy is queued.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "field_plan.hpp"

using namespace usv;

static const char *const ARENA_SET[] = {"x", "u", "x0", "yref", "yref_e", "p", "lh"}; // the arena fields a caller sets and gets

struct Queued { CopyDesc c; bool up; };

struct Sim {
    FieldDims d;
    size_t B;
    HostMirror m;
    std::vector<unsigned char> dev, mir, twin;
    std::vector<Queued> stream;
    bool verbose = true;
    double counter = 0;
    long ngets = 0, nserved = 0, nflush = 0, nwaits = 0, ncopies = 0;
    // model:, B == 1 (property (a)): the device holds rows of the field the mirror has not seen / the one stage set since the last flush
    bool behind[ARENA_FIELDS] = {};
    int one_stage[ARENA_FIELDS];

    [[noreturn]] void fail(const char *what) { fprintf(stderr, "model check failed: %s\n", what); exit(1); }

    void init(bool mirror)
    {
        const ArenaLayout l = arena_layout(d, B);
        m.reset(l, mirror && l.bytes() <= MIRROR_MAX);
        dev.assign(l.bytes(), 0); mir = dev; twin = dev;
        for (int &s : one_stage) s = -1;
    }
    // ---- the executor: a descriptor becomes a copy on the stream; the stream runs when somebody waits for it
    void enqueue(const char *kind, const CopyDesc &c, bool up)
    {
        if (c.off + (c.rows - 1) * c.pitch + c.width > dev.size()) fail("copy past the arena");
        stream.push_back(Queued{c, up});
        ncopies++;
        if (verbose) printf("copy %s off=%zu pitch=%zu width=%zu rows=%zu\n", kind, c.off, c.pitch, c.width, c.rows);
    }
    void drain()
    {
        for (const Queued &q : stream)
            for (size_t r = 0; r < q.c.rows; r++) {
                const size_t o = q.c.off + r * q.c.pitch;
                if (q.up) std::memcpy(&dev[o], &mir[o], q.c.width); else std::memcpy(&mir[o], &dev[o], q.c.width);
            }
        stream.clear();
    }
    void wait() { drain(); m.synced(); }
    bool quiesce() // (mirror_quiesce)
    {
        const bool w = m.must_wait();
        if (w) { wait(); nwaits++; }
        if (!stream.empty()) fail("the host touches the mirror while a copy is queued");
        return w;
    }
    void flush(bool check = true)
    {
        CopyDesc c;
        while (m.next_upload(c)) enqueue("up", c, true);
        nflush++;
        if (!check) return;
        // a flush point: behind the queued copies the device holds what the direct path holds.  (Checked on a copy of the state: the stream stays queued.)
        std::vector<unsigned char> keep_dev = dev, keep_mir = mir;
        const std::vector<Queued> keep = stream;
        drain();
        if (dev != twin) fail("device arena differs from the direct path at a flush point");
        dev = keep_dev; mir = keep_mir; stream = keep;
    }
    // ---- values: every written element is a fresh number
    void fill(unsigned char *p, size_t bytes, bool ints)
    {
        for (size_t i = 0; i < bytes; i += ints ? sizeof(int) : sizeof(double)) {
            counter += 1;
            if (ints) { const int v = (int)counter; std::memcpy(p + i, &v, sizeof v); }
            else std::memcpy(p + i, &counter, sizeof counter);
        }
    }
    // rows of `span` inside field `slot` of an arena-sized buffer <-> a packed host buffer
    void scatter(std::vector<unsigned char> &buf, int slot, const CopyDesc &s, const unsigned char *host)
    {
        for (size_t r = 0; r < s.rows; r++) std::memcpy(&buf[m.lay.off[slot] + s.off + r * s.pitch], host + r * s.width, s.width);
    }
    void gather(const std::vector<unsigned char> &buf, int slot, const CopyDesc &s, unsigned char *host)
    {
        for (size_t r = 0; r < s.rows; r++) std::memcpy(host + r * s.width, &buf[m.lay.off[slot] + s.off + r * s.pitch], s.width);
    }
    // a device-side writer (a kernel on the stream: behind every queued copy): the same fresh values into the device arena and the twin
    void device_write(int slot, const CopyDesc &s)
    {
        drain();
        std::vector<unsigned char> v(s.rows * s.width);
        fill(v.data(), v.size(), FIELD_TABLE[slot].is_int);
        scatter(dev, slot, s, v.data());
        scatter(twin, slot, s, v.data());
        behind[slot] = true;
    }
    CopyDesc whole(int slot) const { return CopyDesc{0, m.lay.len[slot], m.lay.len[slot], 1}; }

    // ---- the operations, as usvmpc.hip performs them
    int copy_field(const char *name, int stage, bool set) // (copy_field behind its size check)
    {
        Field f;
        int rc = resolve(name, stage, d, set, f);
        if (rc == 0 && f.row->slot < 0) { fprintf(stderr, "'%s' is not an arena field\n", name); exit(2); }
        if (rc == 0 && f.n == 0) { if (verbose) printf("op rc=0 served=0 wait=0 empty=1\n"); return 0; }
        if (rc == 0) rc = stage_check(f);
        if (rc) { if (verbose) printf("op rc=%d served=0 wait=0\n", rc); return rc; }
        const int slot = f.row->slot;
        const CopyDesc s = field_span(f, B);
        std::vector<unsigned char> host(s.rows * s.width), want(s.rows * s.width);
        if (set) { fill(host.data(), host.size(), false); scatter(twin, slot, s, host.data()); }
        else { gather(twin, slot, s, want.data()); ngets++; }
        const bool served = set ? m.set_served(slot) : m.get_served(slot);
        bool waited = false;
        if (served) {
            waited = quiesce();
            if (verbose) printf("op rc=0 served=1 wait=%d\n", (int)waited);
            if (set) {
                scatter(mir, slot, s, host.data());
                CopyDesc now;
                if (m.wrote(slot, s, now)) enqueue("now", now, true);
                if (s.rows == 1 && s.width == m.lay.len[slot]) behind[slot] = false; // (the whole field: the mirror is ahead of the device again)
            } else { gather(mir, slot, s, host.data()); nserved++; }
        } else {
            if (verbose) printf("op rc=0 served=0 wait=0\n");
            if (!set) flush(); // (a get of a field with pending writes sees them)
            wait();            // (the copy, synchronised)
            if (set) scatter(dev, slot, s, host.data()); else gather(dev, slot, s, host.data());
        }
        if (!set && host != want) fail("a get differs from the direct path");
        return 0;
    }
    void solve()
    {
        if (verbose) printf("op rc=0\n");
        flush();
        for (int slot : {(int)FLD_X, (int)FLD_U, (int)FLD_STATUS}) device_write(slot, whole(slot));
        CopyDesc c;
        if (m.read_back(c)) {
            enqueue("back", c, false);
            behind[FLD_X] = behind[FLD_U] = behind[FLD_STATUS] = false;
        }
    }
    void status() // usvmpc_solve behind its usvmpc_sync
    {
        wait();
        const bool served = m.get_served(FLD_STATUS);
        if (verbose) printf("op rc=0 served=%d wait=0\n", (int)served);
        if (served) quiesce();
        const size_t o = m.lay.off[FLD_STATUS], n = m.lay.len[FLD_STATUS];
        ngets++;
        if (std::memcmp(&(served ? mir : dev)[o], &twin[o], n) != 0) fail("status differs from the direct path");
    }
    void device_side(const char *what) // advance: x0; the front end: two stages of yref, the whole of p
    {
        if (verbose) printf("op rc=0\n");
        flush();
        if (!std::strcmp(what, "advance")) { device_write(FLD_X0, whole(FLD_X0)); return; }
        Field f;
        for (int stage : {0, d.N - 1})
            if (resolve("yref", stage, d, true, f) == 0 && f.n > 0) device_write(FLD_YREF, field_span(f, B));
        if (m.lay.len[FLD_P]) device_write(FLD_P, whole(FLD_P));
    }
    void devptr()
    {
        if (verbose) printf("op rc=0\n");
        flush();
        m.handed_out();
    }
    void ext(const char *name, int stage)
    {
        Field f;
        if (resolve(name, stage, d, true, f) || f.row->slot < 0 || stage_check(f)) { fprintf(stderr, "bad ext '%s'\n", name); exit(2); }
        if (verbose) printf("op rc=0\n");
        if (f.n > 0) device_write(f.row->slot, field_span(f, B));
    }
    void drop()
    {
        if (verbose) printf("op rc=0\n");
        if (!m.on) return;
        flush();
        wait();
        m.dropped();
    }

    // ---- random interleavings.  Two conditions keep the script inside what the bookkeeping defines (field_plan.hpp, properties (a), (b)):
    //   (b) the external writer never writes a field under a set that is still deferred as a dirty range (B == 1: any set; else a whole-field
    //       set) - with B == 1 it acts only directly after a flush point, with B > 1 it flushes first only when the field has such a range.
    //       Strided stage sets behind a handed-out pointer went up at once: no condition.
    //   (a) with B == 1, while the device holds rows of a field the mirror has not seen (front end, external writer), the per-stage sets of
    //       that field between two flushes all name one stage: its dirty range then covers nothing in between.
    uint64_t rng;
    unsigned rnd(unsigned n) { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)((rng >> 33) % n); }
    void model(uint64_t seed, long ops)
    {
        rng = seed * 2654435761u + 12345;
        verbose = false;
        bool ptr_out = false;
        const long ptr_at = seed % 2 ? ops / 2 : -1;          // (odd seeds hand a device pointer out half way)
        const long drop_at = seed % 3 == 0 ? ops * 3 / 4 : -1; // (every third gives the mirror up on the way)
        for (long i = 0; i < ops; i++) {
            if (i == ptr_at) { devptr(); ptr_out = true; }
            if (i == drop_at) drop();
            const unsigned r = rnd(100);
            const char *name = ARENA_SET[rnd(7)];
            const FieldRow *row = find_field(name);
            const int slot = row->slot, nst = field_stages(*row, d) + (row->id == FLD_YREF ? 1 : 0); // ("yref" reaches stage N: yref_e)
            int stage = rnd(3) == 0 ? -1 : (int)rnd((unsigned)nst);
            const long flushes = nflush;
            if (r < 45) {
                if (B == 1 && stage >= 0 && behind[slot] && m.on) {
                    if (one_stage[slot] < 0) one_stage[slot] = stage;
                    stage = one_stage[slot];
                }
                if (copy_field(name, stage, true)) fail("a set in range was refused");
            } else if (r < 70) {
                if (copy_field(name, stage, false)) fail("a get in range was refused");
            } else if (r < 80) { solve(); if (rnd(2)) { wait(); status(); } }
            else if (r < 85) device_side("advance");
            else if (r < 90) device_side("frontend");
            else if (r < 97) {
                if (!ptr_out) continue;
                Field f = {};
                if (resolve(row, stage, d, true, f)) fail("an arena field did not resolve");
                const int fs = f.row->slot;
                if (m.on && (B == 1 || m.dirty_lo[fs] < m.dirty_hi[fs])) flush();
                ext(name, stage);
            } else wait();
            if (nflush != flushes) for (int &s : one_stage) s = -1;
        }
        flush();
        wait();
        if (dev != twin) fail("device arena differs from the direct path at the end");
        printf("model ok ops=%ld gets=%ld served=%ld flushes=%ld waits=%ld copies=%ld\n", ops, ngets, nserved, nflush, nwaits, ncopies);
    }
};

static std::vector<std::string> split(const std::string &s)
{
    std::vector<std::string> out;
    size_t a = 0;
    for (size_t c; (c = s.find(':', a)) != std::string::npos; a = c + 1) out.push_back(s.substr(a, c - a));
    out.push_back(s.substr(a));
    return out;
}

int main(int argc, char **argv)
{
    Sim S;
    S.d = FieldDims{4, 3, 2, 4, 2, 2, 5, false};
    S.B = 1;
    bool mirror = true, ready = false;
    for (int a = 1; a < argc; a++) {
        const std::string arg = argv[a];
        const size_t eq = arg.find('=');
        if (eq != std::string::npos) {
            const std::string key = arg.substr(0, eq);
            const int v = atoi(arg.c_str() + eq + 1);
            if (key == "exported") { S.d.exported = v != 0; continue; } // (usvmpc.hip: ensure_export; any time)
            if (ready) { fprintf(stderr, "'%s' after the first operation\n", argv[a]); return 2; }
            if (key == "B") S.B = (size_t)v;
            else if (key == "N") S.d.N = v;
            else if (key == "nx") S.d.nx = v;
            else if (key == "nu") S.d.nu = v;
            else if (key == "ny") S.d.ny = v;
            else if (key == "ny_e") S.d.ny_e = v;
            else if (key == "K") S.d.K = v;
            else if (key == "nlam") S.d.nlam = v;
            else if (key == "mirror") mirror = v != 0;
            else { fprintf(stderr, "unknown name '%s'\n", key.c_str()); return 2; }
            continue;
        }
        const std::vector<std::string> t = split(arg);
        if (t[0] == "row" && t.size() == 2) {
            const FieldRow *r = find_field(t[1].c_str());
            if (!r) { printf("row name=%s found=0\n", t[1].c_str()); continue; }
            printf("row name=%s found=1 id=%d slot=%d int=%d set=%d get=%d get_int=%d dev=%d whole=%d lin=%d pf=%d export=%d track=%d\n", r->name, (int)r->id,
                   r->slot, (int)r->is_int, !!(r->rights & R_SET), !!(r->rights & R_GET), !!(r->rights & R_GET_INT), !!(r->rights & R_DEV),
                   !!(r->flags & FF_WHOLE), !!(r->flags & FF_LIN), !!(r->flags & FF_PF), !!(r->flags & FF_EXPORT), !!(r->flags & FF_TRACK));
            continue;
        }
        if (t[0] == "q" && t.size() == 4) {
            Field f;
            const int rc = resolve(t[2].c_str(), atoi(t[3].c_str()), S.d, t[1] == "set", f);
            if (rc) { printf("q rc=%d\n", rc); continue; }
            const CopyDesc s = stage_check(f) ? CopyDesc{0, 0, 0, 0} : field_span(f, S.B);
            printf("q rc=0 as=%s slot=%d n=%d stages=%d stage_off=%d stage=%d check=%d lin=%d pf=%d off=%zu pitch=%zu width=%zu rows=%zu\n", f.row->name,
                   f.row->slot, f.n, f.stages, f.stage_off, f.stage, stage_check(f), !!(f.row->flags & FF_LIN), !!(f.row->flags & FF_PF), s.off, s.pitch,
                   s.width, s.rows);
            continue;
        }
        if (!ready) { S.init(mirror); ready = true; }
        if (t[0] == "layout") {
            for (int s = 0; s < ARENA_FIELDS; s++) printf("layout name=%s off=%zu len=%zu stages=%zu\n", FIELD_TABLE[s].name, S.m.lay.off[s], S.m.lay.len[s], S.m.lay.stages[s]);
            printf("layout name=end off=%zu len=0 stages=0 mirrored=%d max=%zu\n", S.m.lay.bytes(), (int)S.m.on, MIRROR_MAX);
        }
        else if ((t[0] == "set" || t[0] == "get") && t.size() == 3) S.copy_field(t[1].c_str(), atoi(t[2].c_str()), t[0] == "set");
        else if (t[0] == "flush") { if (S.verbose) printf("op rc=0\n"); S.flush(); }
        else if (t[0] == "solve") S.solve();
        else if (t[0] == "status") S.status();
        else if (t[0] == "advance" || t[0] == "frontend") S.device_side(t[0].c_str());
        else if (t[0] == "devptr") S.devptr();
        else if (t[0] == "ext" && t.size() == 3) S.ext(t[1].c_str(), atoi(t[2].c_str()));
        else if (t[0] == "sync") { if (S.verbose) printf("op rc=0\n"); S.wait(); }
        else if (t[0] == "drop") S.drop();
        else if (t[0] == "model" && t.size() == 3) S.model((uint64_t)atoll(t[1].c_str()), atol(t[2].c_str()));
        else { fprintf(stderr, "bad argument '%s'\n", argv[a]); return 2; }
    }
    if (ready) { S.verbose = false; S.flush(); S.wait(); } // (a script ends at a flush point)
    return 0;
}
