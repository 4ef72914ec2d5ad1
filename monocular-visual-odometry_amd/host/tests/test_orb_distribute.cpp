// host/tests/test_orb_distribute.cpp -- drives Frame::calcKeyPoints / calcDescriptors of the mirror with the key
// `orb_distribute_keypoints` as given (my_slam/geometry/orb_distribute.h, my_slam/vo/frame.h) and dumps the results next to those
// of the C-ABI called directly, for tests/test_orb_distribute_host.py.
//   test_orb_distribute <image.bin> <out.bin> [key=value ...]
// image.bin: int32 w, h, channels; then h * w * channels bytes.  key=value pairs are set in basics::Config before anything is
// latched.
// out.bin (each a uint64 count followed by the items): the key points of Frame::calcKeyPoints; the candidates per level and the
// key points per level it recorded (none with the key off); the key points and the descriptors after Frame::calcDescriptors; the
// key points of mvo_calc_keypoints_distributed and of mvo_calc_keypoints called directly on the same context afterwards.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "my_slam/vo/frame.h"

using namespace my_slam;

template <class T>
static void dump(std::ofstream& o, const T* p, size_t n) {
    unsigned long long cnt = n;
    o.write(reinterpret_cast<const char*>(&cnt), 8);
    o.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T)));
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    for (int a = 3; a < argc; ++a) {
        const string kv = argv[a];
        const size_t eq = kv.find('=');
        if (eq == string::npos) return 2;
        basics::Config::set(kv.substr(0, eq), kv.substr(eq + 1));
    }
    int hdr[3];
    if (!in.read(reinterpret_cast<char*>(hdr), sizeof hdr)) return 2;
    const int w = hdr[0], h = hdr[1], ch = hdr[2];
    try {
        cv::Mat img(h, w, ch == 3 ? CV_8UC3 : CV_8UC1);
        if (!in.read(reinterpret_cast<char*>(img.data), (std::streamsize)((size_t)w * h * ch))) return 2;
        vo::Frame::Ptr f = vo::Frame::createFrame(img);
        f->calcKeyPoints();
        dump(out, f->keypoints_.data(), f->keypoints_.size());
        dump(out, f->distribute_candidates_per_level_.data(), f->distribute_candidates_per_level_.size());
        dump(out, f->distribute_keypoints_per_level_.data(), f->distribute_keypoints_per_level_.size());
        f->calcDescriptors();
        dump(out, f->keypoints_.data(), f->keypoints_.size());
        dump(out, f->descriptors_.data, (size_t)f->descriptors_.rows * 32);
        // the C-ABI itself, on the context the mirror has configured
        const int cap = basics::Config::get<int>("max_number_of_keypoints") + 16;
        vector<mvo_keypoint> k(cap);
        int n = 0;
        mvo_check(mvo_calc_keypoints_distributed(hot_path_ctx(), img.data, w, h, (int)img.step, ch, k.data(), cap, &n), "mvo_calc_keypoints_distributed");
        dump(out, k.data(), (size_t)n);
        mvo_check(mvo_calc_keypoints(hot_path_ctx(), img.data, w, h, (int)img.step, ch, k.data(), cap, &n), "mvo_calc_keypoints");
        dump(out, k.data(), (size_t)n);
    } catch (const std::exception& e) {
        fprintf(stderr, "test_orb_distribute: %s\n", e.what());
        return 1;
    }
    return 0;
}
