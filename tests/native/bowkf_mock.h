// The mock KeyFrame / MapPoint graph and the accessor of the SearchByBoW(KF, KF) / LoopBowProblems shim checks
// (bowkf_shim_check.cpp on ABI test doubles, bowkf_shim_gpu.cpp on the real library).
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "orbgpu.h"

struct MockKF;
struct MockMP {
    float pos[3] = {0, 0, 4};
    bool bad = false;
    std::map<MockKF*, int> obs;  // GetIndexInKeyFrame
};
struct MockKF {
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> desc;
    std::vector<MockMP*> mps;
    std::map<unsigned, std::vector<unsigned>> fv;
    std::vector<float> scale, sigma2;
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    float K[4] = {458.654f, 457.296f, 367.215f, 248.375f};
    bool bad = false;
    MockKF() {
        for (int l = 0; l < 8; ++l) {
            scale.push_back(l ? scale.back() * 1.2f : 1.f);
            sigma2.push_back(scale.back() * scale.back());
        }
    }
    // a feature whose 32 descriptor bytes are `code`, under FeatureVector node `node`
    int add(unsigned node, uint8_t code, MockMP* mp, int octave = 0, float angle = 0.f, bool observed = true) {
        orb_keypoint_t k{};
        k.octave = octave;
        k.angle = angle;
        kps.push_back(k);
        desc.resize(desc.size() + 32, code);
        mps.push_back(mp);
        const int i = (int)kps.size() - 1;
        fv[node].push_back((unsigned)i);
        if (mp && observed) mp->obs[this] = i;
        return i;
    }
};

struct Mat4 { float m[16]; };
struct Mat3 { float m[9]; };
struct Vec3 { float v[3]; };

extern int g_random_calls;

struct Access {
    using KeyFrame = MockKF;
    using MapPoint = MockMP;
    struct Frame {};
    using Matrix4f = Mat4;
    using Matrix3f = Mat3;
    using Vector3f = Vec3;
    static Mat4 Matrix4(const float m[16]) { Mat4 r; std::memcpy(r.m, m, 64); return r; }
    static Mat3 Matrix3(const float m[9]) { Mat3 r; std::memcpy(r.m, m, 36); return r; }
    static Vec3 Vector3(const float v[3]) { Vec3 r; std::memcpy(r.v, v, 12); return r; }
    static int N(KeyFrame* k) { return (int)k->kps.size(); }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return k->kps.data(); }
    static const uint8_t* Descriptors(KeyFrame* k) { return k->desc.data(); }
    static const float* URight(KeyFrame*) { return nullptr; }
    static std::vector<MapPoint*> MapPointMatches(KeyFrame* k) { return k->mps; }
    static const std::map<unsigned, std::vector<unsigned>>& FeatVec(KeyFrame* k) { return k->fv; }
    static void Pinhole(KeyFrame* k, float K[4]) { std::memcpy(K, k->K, 16); }
    static int Levels(KeyFrame* k) { return (int)k->scale.size(); }
    static const float* ScaleFactors(KeyFrame* k) { return k->scale.data(); }
    static const float* LevelSigma2(KeyFrame* k) { return k->sigma2.data(); }
    static bool SingleCamera(KeyFrame*) { return true; }
    static bool IsBad(MapPoint* p) { return p->bad; }
    static bool IsBad(KeyFrame* k) { return k->bad; }
    static int IndexInKeyFrame(MapPoint* p, KeyFrame* k) {
        auto it = p->obs.find(k);
        return it == p->obs.end() ? -1 : it->second;
    }
    static void Pose(KeyFrame* k, float R[9], float t[3]) {
        std::memcpy(R, k->R, 36);
        std::memcpy(t, k->t, 12);
    }
    static void WorldPos(MapPoint* p, float X[3]) { std::memcpy(X, p->pos, 12); }
    static int RandomInt(int lo, int hi) {  // a fixed linear congruential stream
        static unsigned s = 12345u;
        ++g_random_calls;
        s = s * 1664525u + 1013904223u;
        return lo + (int)((s >> 8) % (unsigned)(hi - lo + 1));
    }
};
