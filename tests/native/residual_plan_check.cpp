// CPU check of the residual report's host plan (tscm_calib_amd/csrc/tscm_residual_plan.h).  Host logic only (no GPU).
//   usage: residual_plan_check plan < problems    one JSON line: every table of plan_residuals for each problem on standard
//          input, and "ok": the invariants checked here -- every view with corners in exactly one chunk, views ascending
//          within a chunk and a camera's chunks in order, one camera per chunk, no chunk above the target unless it is a
//          single view, a closed chunk could not have taken the next view, view_first the prefix sum of view_count.
//          Input, integers separated by white space: the number of problems, then per problem
//            C V target, V x (camera corners)
//          residual_plan_check refuse           one JSON line: plan_residuals' refusals, checked here
#include "../../tscm_calib_amd/csrc/tscm_residual_plan.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace tscm;

template <typename T>
static void put(const char *name, const std::vector<T> &v, bool last = false)
{
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? ", " : "", (long long)v[i]);
    std::printf("]%s", last ? "" : ", ");
}

static bool invariants(const ResidualPlan &r, int C, int V, const std::vector<int> &cam, const std::vector<int> &count, int target)
{
    if (target <= 0) target = kResidualChunkTarget;
    if ((int)r.view_first.size() != V + 1 || r.view_first[0] != 0) return false;
    for (int v = 0; v < V; ++v)
        if (r.view_first[v + 1] - r.view_first[v] != count[v]) return false;
    if (r.N != r.view_first[V]) return false;
    if ((int)r.cam_start.size() != C + 1 || r.cam_start[C] != V || (int)r.cam_views.size() != V) return false;
    std::vector<int> seen((size_t)V, 0);
    for (int m = 0; m < C; ++m)
        for (int k = r.cam_start[m]; k < r.cam_start[m + 1]; ++k) {
            const int v = r.cam_views[k];
            if (v < 0 || v >= V || cam[v] != m || seen[v]++) return false;
            if (k > r.cam_start[m] && r.cam_views[k - 1] >= v) return false;
        }
    const size_t n = r.chunk_begin.size();
    if (r.chunk_end.size() != n || r.chunk_camera.size() != n) return false;
    std::vector<int> in_chunk((size_t)V, 0);
    int at = 0;
    for (size_t c = 0; c < n; ++c) {
        if (r.chunk_begin[c] != at || r.chunk_end[c] <= r.chunk_begin[c] || r.chunk_end[c] > (int)r.field_views.size()) return false;
        if (c && r.chunk_camera[c] < r.chunk_camera[c - 1]) return false;
        long long corners = 0;
        for (int k = r.chunk_begin[c]; k < r.chunk_end[c]; ++k) {
            const int v = r.field_views[k];
            if (v < 0 || v >= V || count[v] == 0 || cam[v] != r.chunk_camera[c]) return false;
            if (k > r.chunk_begin[c] && r.field_views[k - 1] >= v) return false;
            in_chunk[v]++;
            corners += count[v];
        }
        if (corners > target && r.chunk_end[c] - r.chunk_begin[c] != 1) return false;
        // a chunk closed ahead of a view of the same camera could not have taken it
        if (c + 1 < n && r.chunk_camera[c + 1] == r.chunk_camera[c]) {
            if (r.field_views[r.chunk_begin[c + 1]] <= r.field_views[r.chunk_end[c] - 1]) return false;
            if (corners + count[r.field_views[r.chunk_begin[c + 1]]] <= target) return false;
        }
        at = r.chunk_end[c];
    }
    if (at != (int)r.field_views.size()) return false;
    for (int v = 0; v < V; ++v)
        if (in_chunk[v] != (count[v] > 0 ? 1 : 0)) return false;
    return true;
}

static int plan_mode()
{
    int n = 0;
    if (!(std::cin >> n)) return 2;
    std::printf("[");
    for (int k = 0; k < n; ++k) {
        int C, V, target;
        if (!(std::cin >> C >> V >> target)) return 2;
        std::vector<int> cam(V), count(V);
        for (int v = 0; v < V; ++v) std::cin >> cam[v] >> count[v];
        if (!std::cin) return 2;
        ResidualPlan r;
        std::string err;
        const int rc = plan_residuals(C, V, cam.data(), count.data(), target, r, err);
        std::printf("%s{\"rc\": %d, \"ok\": %s, \"N\": %lld, ", k ? ", " : "", rc, rc == 0 && invariants(r, C, V, cam, count, target) ? "true" : "false", r.N);
        put("view_first", r.view_first); put("cam_start", r.cam_start); put("cam_views", r.cam_views); put("cam_corners", r.cam_corners);
        put("field_views", r.field_views); put("chunk_camera", r.chunk_camera); put("chunk_begin", r.chunk_begin); put("chunk_end", r.chunk_end, true);
        std::printf("}");
    }
    std::printf("]\n");
    return 0;
}

static int refuse_mode()
{
    const int cam[3] = { 0, 1, 0 }, count[3] = { 4, 4, 4 }, bad_cam[3] = { 0, 2, 0 }, bad_count[3] = { 4, -1, 4 };
    struct Case { const char *name; int C, V; const int *cam, *count; const char *text; };
    const Case cases[] = {
        { "no_cameras", 0, 3, cam, count, "n_cameras" },       { "too_many_cameras", 33, 3, cam, count, "n_cameras" },
        { "negative_views", 2, -1, cam, count, "n_views" },    { "null_camera", 2, 3, nullptr, count, "view_camera is NULL" },
        { "null_count", 2, 3, cam, nullptr, "view_count is NULL" }, { "camera_range", 2, 3, bad_cam, count, "view_camera[1]" },
        { "negative_count", 2, 3, cam, bad_count, "view_count[1]" },
    };
    bool all = true;
    std::printf("{");
    for (const Case &c : cases) {
        ResidualPlan r;
        r.C = -7;                                              // a refusal leaves the output untouched
        std::string err;
        const int rc = plan_residuals(c.C, c.V, c.cam, c.count, 0, r, err);
        const bool ok = rc == TSCM_E_INVALID && err.find(c.text) != std::string::npos && r.C == -7;
        all = all && ok;
        std::printf("\"%s\": %s, ", c.name, ok ? "true" : "false");
    }
    std::printf("\"all\": %s}\n", all ? "true" : "false");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "plan")) return plan_mode();
    if (argc == 2 && !std::strcmp(argv[1], "refuse")) return refuse_mode();
    std::fprintf(stderr, "usage: residual_plan_check plan|refuse\n");
    return 2;
}
