// tscm::findCorners of include/tscm/tscm_calib.hpp (one detector batch, one recovery batch) against tscm::findCorner per image:
//   mirror_boards device|host sigma a.pgm b.pgm ...      (8-bit binary PGMs of one size)
// prints per image "image k candidates N boards B same S" and the points of board 0 in board order (%.17g); status 1 when
// an image differs in a candidate, a board or a point.
#include <tscm/tscm_calib.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool read_pgm(const char *path, std::vector<unsigned char> &img, int &w, int &h)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    int maxv = 0;
    const bool ok = std::fscanf(f, "P5 %d %d %d", &w, &h, &maxv) == 3 && maxv == 255 && std::fgetc(f) != EOF;
    if (ok) img.resize((size_t)w * h);
    const bool all = ok && std::fread(img.data(), 1, img.size(), f) == img.size();
    std::fclose(f);
    return all;
}

static bool same(const tscm::Chessboarder_t &a, const tscm::Chessboarder_t &b)
{
    if (a.corners.p.size() != b.corners.p.size() || a.chessboard.size() != b.chessboard.size()) return false;
    for (size_t i = 0; i < a.corners.p.size(); ++i)
        if (a.corners.p[i].x != b.corners.p[i].x || a.corners.p[i].y != b.corners.p[i].y || a.corners.score[i] != b.corners.score[i]) return false;
    for (size_t q = 0; q < a.chessboard.size(); ++q)
        if (a.chessboard[q].rows != b.chessboard[q].rows || a.chessboard[q].cols != b.chessboard[q].cols || a.chessboard[q].data != b.chessboard[q].data) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s device|host sigma image.pgm ...\n", argv[0]); return 2; }
    const int where = std::strcmp(argv[1], "host") == 0 ? TSCM_BOARDS_HOST : TSCM_BOARDS_DEVICE, sigma = std::atoi(argv[2]);
    std::vector<std::vector<unsigned char> > imgs((size_t)argc - 3);
    std::vector<const unsigned char *> ptrs;
    int w = 0, h = 0;
    for (int k = 3; k < argc; ++k) {
        int wk = 0, hk = 0;
        if (!read_pgm(argv[k], imgs[(size_t)k - 3], wk, hk) || (k > 3 && (wk != w || hk != h))) { std::fprintf(stderr, "cannot use %s\n", argv[k]); return 2; }
        w = wk; h = hk;
        ptrs.push_back(imgs[(size_t)k - 3].data());
    }
    try {
        const std::vector<tscm::Chessboarder_t> batch = tscm::findCorners(ptrs, w, h, w, sigma, 0, where);
        bool all = batch.size() == ptrs.size();
        for (size_t k = 0; k < batch.size(); ++k) {
            const tscm::Chessboarder_t one = tscm::findCorner(ptrs[k], w, h, w, sigma);
            const bool s = same(batch[k], one);
            all = all && s;
            std::printf("image %d candidates %d boards %d same %d\n", (int)k, (int)batch[k].corners.p.size(), (int)batch[k].chessboard.size(), s ? 1 : 0);
            if (batch[k].chessboard.empty()) continue;
            const tscm::IndexMat &m = batch[k].chessboard[0];
            for (size_t q = 0; q < m.data.size(); ++q) std::printf("%.17g %.17g\n", batch[k].corners.p[m.data[q]].x, batch[k].corners.p[m.data[q]].y);
        }
        return all ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
