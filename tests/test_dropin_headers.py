"""The drop-in claim, checked against the reference's OWN headers: the two translation
units host/src/feature_match_mvo.cpp and host/src/g2o_ba_mvo.cpp replace src/geometry/feature_match.cpp and
src/optimization/g2o_ba.cpp of the reference -- compiled with -I /root/reference/include UNMODIFIED, no header of the reference
shadowed (this repo's my_slam/ mirror is NOT on the include path here).  OpenCV is not installed in this image: the cv:: names
come from tests/stub_cv/ (a test aid routing to the mirror's layout-compatible mini_cv.h).  Reference translation units that
call into the replaced functions or define the types around them (src/vo/frame.cpp, map.cpp, mappoint.cpp, the
createFrame(rgb_img, camera) call of run_vo.cpp:122) are syntax-checked against the same include path."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

REF = "/root/reference"
HOST = os.path.join(ROOT, "monocular-visual-odometry_amd", "host")
INC = ["-I", os.path.join(REF, "include"), "-I", os.path.join(ROOT, "tests", "stub_cv"), "-I", os.path.join(ROOT, "include"),
       "-I", os.path.join(HOST, "src")]
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "my_slam")),
                                     reason="needs a checkout of the reference project (its include/ and src/)")


def gxx(args, **kw):
    return subprocess.run(["g++", "-std=c++17", "-Wall"] + INC + args, capture_output=True, text=True, **kw)


def test_include_path_holds_no_mirror_header():
    """Nothing named my_slam/* may come from this repo on that path: include/ holds mvo_hip.h only, host/src/ only the two
    private helpers and the translation units."""
    for d in (os.path.join(ROOT, "include"), os.path.join(HOST, "src"), os.path.join(ROOT, "tests", "stub_cv")):
        assert not os.path.exists(os.path.join(d, "my_slam")), d
    assert sorted(f for f in os.listdir(os.path.join(HOST, "src")) if f.endswith((".h", ".cpp"))) == [
        "feature_match_mvo.cpp", "flat_bundle.h", "g2o_ba_mvo.cpp", "mvo_hot_path.h"]


@needs_reference
@pytest.mark.parametrize("tu", ["feature_match_mvo.cpp", "g2o_ba_mvo.cpp"])
def test_translation_units_compile_against_the_reference_headers(tu, tmp_path):
    obj = str(tmp_path / (tu + ".o"))
    r = gxx(["-c", os.path.join(HOST, "src", tu), "-o", obj, "-H"])
    assert r.returncode == 0, r.stderr[-3000:]
    # the my_slam headers it saw are the reference's (-H lists every header opened)
    # (mini_cv.h is the stub tree's stand-in for the OpenCV value types, reached by relative path from tests/stub_cv)
    seen = [l.strip(". \n") for l in r.stderr.splitlines() if "my_slam/" in l and l.startswith(".") and not l.rstrip().endswith("mini_cv.h")]
    assert seen and all(s.startswith(REF + "/include/my_slam/") for s in seen), seen


@needs_reference
def test_the_eleven_functions_and_nothing_else_of_the_reference_interface(tmp_path):
    """feature_match.h:12-54 declares nine functions, g2o_ba.h:16-30 two: the translation units define exactly those in
    my_slam::geometry / my_slam::optimization (plus private helpers in my_slam::geometry::detail)."""
    want = {"calcKeyPoints", "calcDescriptors", "matchFeatures", "matchByRadiusAndBruteForce", "removeDuplicatedMatches",
            "selectUniformKptsByGrid", "computeMeanDistBetweenKeypoints", "inliers2DMatches", "pts2Keypts",
            "optimizeSingleFrame", "bundleAdjustment"}
    # the declarations of the reference headers themselves
    decl = set()
    for h in ("geometry/feature_match.h", "optimization/g2o_ba.h"):
        src = open(os.path.join(REF, "include", "my_slam", h)).read()
        src = re.sub(r"//[^\n]*|/\*.*?\*/", "", src, flags=re.S)
        decl |= set(re.findall(r"\b(\w+)\s*\(", src)) & want
    assert decl == want
    got = set()
    for tu in ("feature_match_mvo.cpp", "g2o_ba_mvo.cpp"):
        obj = str(tmp_path / (tu + ".o"))
        assert gxx(["-c", os.path.join(HOST, "src", tu), "-o", obj]).returncode == 0
        for line in subprocess.run(["nm", "-C", "--defined-only", obj], capture_output=True, text=True).stdout.splitlines():
            m = re.search(r" T my_slam::(geometry|optimization)::(\w+)\(", line)
            if m:
                got.add(m.group(2))
    assert got == want, (sorted(got - want), sorted(want - got))


@needs_reference
@pytest.mark.parametrize("src", ["src/vo/frame.cpp", "src/vo/map.cpp", "src/vo/mappoint.cpp"])
def test_reference_sources_around_the_hot_path_still_parse(src):
    r = gxx(["-fsyntax-only", os.path.join(REF, src)])
    assert r.returncode == 0, r.stderr[-3000:]


@needs_reference
def test_run_vo_call_shape(tmp_path):
    """run_vo.cpp:117-126: imread -> Frame::createFrame(rgb_img, camera) -> the frame's extraction; vo.cpp:283 / 458: the calls
    into the two replaced translation units with the argument types of the reference's call sites."""
    f = tmp_path / "call_shape.cpp"
    f.write_text(r'''
#include "my_slam/vo/frame.h"
#include "my_slam/vo/map.h"
#include "my_slam/optimization/g2o_ba.h"
using namespace my_slam;
void per_frame(cv::Mat rgb_img, geometry::Camera::Ptr camera, vo::Frame::Ptr ref, vo::Map::Ptr map) {
    vo::Frame::Ptr frame = vo::Frame::createFrame(rgb_img, camera);       // run_vo.cpp:122
    frame->calcKeyPoints();                                                // frame.h:73-76
    frame->calcDescriptors();                                              // frame.h:77-86
    geometry::matchFeatures(ref->descriptors_, frame->descriptors_, frame->matches_with_ref_, 1, false,
                            ref->keypoints_, frame->keypoints_, 50.0f);   // vo.cpp:283, vo_addFrame.cpp:42,99
    (void)frame->isInFrame(cv::Point3f(0, 0, 1));                          // vo.cpp:496
    (void)frame->getCamCenter();                                           // vo.cpp:563
    vector<vector<cv::Point2f *>> v_pts_2d(1);
    vector<vector<int>> v_pts_2d_to_3d_idx(1);
    std::unordered_map<int, cv::Point3f *> pts_3d;
    vector<cv::Mat *> v_camera_poses{&frame->T_w_c_};
    cv::Mat information_matrix = (cv::Mat_<double>(2, 2) << 1, 0, 0, 1);
    optimization::bundleAdjustment(v_pts_2d, v_pts_2d_to_3d_idx, frame->camera_->K_, pts_3d, v_camera_poses,
                                   information_matrix, false, true);     // vo.cpp:458-462
}
''')
    r = gxx(["-fsyntax-only", str(f)])
    assert r.returncode == 0, r.stderr[-3000:]
    # the same call sites as a program of this repo (host/tests/test_callsites.cpp), against the reference's headers
    r = gxx(["-fsyntax-only", os.path.join(HOST, "tests", "test_callsites.cpp")])
    assert r.returncode == 0, r.stderr[-3000:]
