// heatray_amd/csrc/hr_deform.h on the CPU (tests/test_deform_ref.py, also built with -fsanitize=address,undefined): the functions
// k_deform_pose compiles, over one rig read from a file.  All words are 4 bytes.
// Input: int32 V, K (morphs), J (joints), flags (1: morph normals, 2: tangent frames); then restP, restN (V x 3 each), with flag 2 restT,
// restB; dP (K x V x 3), with flag 1 dN; with J > 0 joints (V x 4 uint32) and weights (V x 4); 8 morph weights; J x 16 matrix words.
// Output: V records of p, n, t, b (12 floats), then rejected and kept (uint32).
#include "hr_deform.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace hr;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hd[4];
    if (fread(hd, 4, 4, f) != 4) return 4;
    const size_t V = (size_t)hd[0], K = (size_t)hd[1], J = (size_t)hd[2];
    const bool morphN = (hd[3] & 1) != 0, frames = (hd[3] & 2) != 0;
    if (hd[0] < 0 || hd[1] < 0 || hd[1] > 8 || hd[2] < 0 || hd[2] > 1024) return 4;
    const auto read = [&](std::vector<float> &a, size_t words) {
        a.resize(words);
        return words == 0 || fread(a.data(), 4, words, f) == words;
    };
    std::vector<float> restP, restN, restT, restB, dP, dN, weights, pose, mats;
    std::vector<uint32_t> joints(J ? 4 * V : 0);
    bool ok = read(restP, 3 * V) && read(restN, 3 * V) && read(restT, frames ? 3 * V : 0) && read(restB, frames ? 3 * V : 0);
    ok = ok && read(dP, K * V * 3) && read(dN, morphN ? K * V * 3 : 0);
    ok = ok && (joints.empty() || fread(joints.data(), 4, joints.size(), f) == joints.size()) && read(weights, J ? 4 * V : 0);
    ok = ok && read(pose, 8) && read(mats, J * 16);
    fclose(f);
    if (!ok) return 5;
    for (uint32_t j : joints)
        if (j >= J) return 7; // (hr_deform_bind's check: the function indexes the matrices unchecked)
    DfRig<const float *, const uint32_t *> r;
    r.dP = K ? dP.data() : nullptr, r.dN = morphN && K ? dN.data() : nullptr, r.joints = joints.data(), r.weights = weights.data();
    r.morphW = pose.data(), r.mats = mats.data(), r.V = (uint32_t)V, r.nMorph = (int32_t)K, r.nJoints = (int32_t)J;
    std::vector<float> out;
    uint32_t rejected = 0, kept = 0;
    for (size_t v = 0; v < V; ++v) {
        bool keep;
        const v3 zero(0.0f);
        const v3 p = dfPosePosition(r, (uint32_t)v, dfLoad3(restP.data(), v), keep);
        rejected += keep;
        // what hr_deform_pose does not write comes out as the rest value (0 for the frames of a mesh without them)
        v3 n = dfLoad3(restN.data(), v), t = frames ? dfLoad3(restT.data(), v) : zero, b = frames ? dfLoad3(restB.data(), v) : zero;
        if (morphN || J) n = dfPoseNormal(r, (uint32_t)v, n, keep), kept += keep;
        if (frames && J) {
            t = dfPoseFrame(r, (uint32_t)v, t, keep), kept += keep;
            b = dfPoseFrame(r, (uint32_t)v, b, keep), kept += keep;
        }
        for (const v3 &x : {p, n, t, b}) out.push_back(x.x), out.push_back(x.y), out.push_back(x.z);
    }
    float w[2];
    memcpy(&w[0], &rejected, 4), memcpy(&w[1], &kept, 4);
    out.push_back(w[0]), out.push_back(w[1]);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 6;
    fclose(f);
    printf("deform cpu: ok\n");
    return 0;
}
