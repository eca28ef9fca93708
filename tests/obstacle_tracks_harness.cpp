// The arithmetic of the obstacle tracks (csrc/obstacle_tracks.hpp) on the host.  Command line: "B N K dt T nx ipx ipy in out".  `in` holds
// doubles pos [B][2K], vel [B][2K], x0 [B][nx], lh [B][K]; `out` receives p [B][N+1][2K] (track_predict, laid out as the device lays it
// out), the stepped positions [B][2K] (track_step by T) and the clearance [B] of x0's position against the STEPPED obstacles
// (track_clearance) - what usv_obstacle_predict / usv_obstacle_step compute with the same functions.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "obstacle_tracks.hpp"

int main(int argc, char **argv)
{
    if (argc != 11) return 2;
    const long B = atol(argv[1]);
    const int N = atoi(argv[2]), K = atoi(argv[3]);
    const double dt = atof(argv[4]), T = atof(argv[5]);
    const int nx = atoi(argv[6]), ipx = atoi(argv[7]), ipy = atoi(argv[8]);
    std::vector<double> pos(B * 2 * K), vel(B * 2 * K), x0(B * nx), lh(B * K);
    FILE *f = fopen(argv[9], "rb");
    if (!f) return 3;
    const bool ok = fread(pos.data(), 8, pos.size(), f) == pos.size() && fread(vel.data(), 8, vel.size(), f) == vel.size() &&
                    fread(x0.data(), 8, x0.size(), f) == x0.size() && fread(lh.data(), 8, lh.size(), f) == lh.size();
    fclose(f);
    if (!ok) return 4;
    std::vector<double> p(B * (N + 1) * 2 * K), stepped(B * 2 * K), clear(B);
    for (long b = 0; b < B; b++) {
        for (int k = 0; k <= N; k++)
            for (int j = 0; j < 2 * K; j++) p[(b * (N + 1) + k) * 2 * K + j] = usv::track_predict(pos[b * 2 * K + j], vel[b * 2 * K + j], k, dt);
        for (int j = 0; j < 2 * K; j++) stepped[b * 2 * K + j] = usv::track_step(pos[b * 2 * K + j], vel[b * 2 * K + j], T);
        clear[b] = usv::track_clearance(x0[b * nx + ipx], x0[b * nx + ipy], &stepped[b * 2 * K], &lh[b * K], K);
    }
    f = fopen(argv[10], "wb");
    if (!f) return 5;
    fwrite(p.data(), 8, p.size(), f);
    fwrite(stepped.data(), 8, stepped.size(), f);
    fwrite(clear.data(), 8, clear.size(), f);
    fclose(f);
    printf("ok %ld\n", B);
    return 0;
}
