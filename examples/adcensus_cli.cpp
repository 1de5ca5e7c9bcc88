// adcensus_cli.cpp -- counterpart of the reference's demo (main.cpp:34-145) without OpenCV:
//   adcensus_cli left.{png,ppm} right.{png,ppm} [min_disparity] [max_disparity] [out_prefix]
// loads the pair (8-bit PNG: gray / RGB / palette / RGBA, non-interlaced; or binary PPM), runs
// ADCensusStereo::Initialize / Match exactly like main.cpp:80-118 and writes what SaveDisparityMap /
// SaveDisparityCloud write (main.cpp:120-128,180-230):
//   <out>-d.png      min-max normalised 8-bit disparity: uchar((|d| - min) / (max - min) * 255), invalid -> 0
//   <out>-c.png      cv::applyColorMap(<out>-d, COLORMAP_JET)
//   <out>-cloud.txt  "x y |d| r g b" per valid pixel ("%f %f %f %d %d %d", colours of the LEFT image)
// plus <out>.pfm (raw float32 disparity, for bit-exact comparisons).  PNG coding uses zlib (the image has no OpenCV).
// --extras (anywhere after the program name) also writes the per-pixel maps of ADCensusStereo::MatchEx:
//   <out>-prov.png   provenance codes (lr | fill << 2, include/adcensus_c_api.h) as 8-bit gray
//   <out>-conf.png   uchar(confidence * 255);  <out>-conf.pfm  the float32 confidence
// --calib f,B,cx,cy,doffs (anywhere after the program name; Middlebury calib.txt convention, not together with --extras) also
// writes the device-side outputs of ADCensusStereo::MatchOut:
//   <out>-depth.pfm  float32 depth Z = f * B / (|d| + doffs), +inf where invalid
//   <out>-cloud.ply  binary little-endian PLY of the valid pixels in raster order: x y z float, red green blue uchar
// --voxel LEAF[,ZMIN,ZMAX] (anywhere after the program name; needs --calib) switches the device-side voxel-grid filter of the cloud on
// (ADCensusStereo::SetCloudVoxelGrid): <out>-cloud.ply and <out>-cloud.txt ("x y z r g b") then hold one point per occupied voxel of edge
// LEAF (the unit of the calibration's baseline) among the points with ZMIN <= Z <= ZMAX (default: 0 and +inf).
// --normals R[,DIFF[,MIN]] (anywhere after the program name; needs --calib) computes camera-facing surface normals from the run's
// disparity map on the device (ADCensusStereo::Normals: a plane fit over the (2R+1) x (2R+1) window, R in 1..7, among the taps within
// DIFF pixels of disparity of the centre, default 1, needing at least MIN of them, default 5): <out>-n.png holds the normal map
// (R, G, B = 128 + 127 * nx, ny, nz; black where there is no normal), and without --voxel the points of <out>-cloud.ply gain the float
// properties nx ny nz (0 0 0 for a point without a normal).  A malformed flag is refused while the arguments are parsed.
// --mesh DIFF[,STEP] (anywhere after the program name; does not need --calib) triangulates the run's disparity map on the device
// (ADCensusStereo::Mesh: gated grid cells over the lattice of every STEP-th pixel, STEP in 1..16, default 1; two lattice pixels are joined
// when their disparities differ by at most DIFF >= 0, inf = no gate) and writes <out>-mesh.ply, a binary little-endian PLY: element
// vertex with x y z float (without --calib x, y, |d|), nx ny nz float only with --normals (gathered through the mesh's vertex_index; 0 0 0
// where there is no normal), red green blue uchar; element face with property list uchar int vertex_indices.  The mesh comes from the
// map, so --voxel does not touch it and with --speckle it has the filter's holes.  A malformed flag is refused while the arguments are
// parsed.
// --tsdf NX,NY,NZ,VOXEL,OX,OY,OZ[,TRUNC[,MINW]] (anywhere after the program name; needs --calib) fuses the run's disparity map and left
// image into a TSDF volume on the device (ADCensusStereo::TsdfCreate / TsdfIntegrate / TsdfExtract: NX x NY x NZ voxels of edge VOXEL,
// NX a multiple of 4, the corner of voxel (0, 0, 0) at the world position OX, OY, OZ, truncation TRUNC, default 3 * VOXEL, a colour
// volume) and writes the surface points between voxels of weight >= MINW, default 1, to <out>-tsdf.ply, a binary little-endian PLY:
// element vertex with x y z float, red green blue uchar, in the world frame.  --pose FILE (only with --tsdf): FILE holds 12 numbers, R
// row-major then t, which take a world point into the left camera (Xc = R * Xw + t); default: the identity.  A malformed flag or file
// is refused while the arguments are parsed.
// --tsdf-mesh (only with --tsdf; refused otherwise while the arguments are parsed) also writes the volume's surface as a triangle mesh
// (ADCensusStereo::TsdfMesh: marching cubes on the device) to <out>-tsdf-mesh.ply, a binary little-endian PLY: the vertex element as in
// <out>-tsdf.ply, then element face with property list uchar int vertex_indices; and prints one line with the report's five counts.
// --tsdf-raycast W,H,F,CX,CY[,STEP[,SKIP]] (only with --tsdf; refused otherwise while the arguments are parsed) also ray-casts the volume
// (ADCensusStereo::TsdfRaycast) into a view of W x H pixels with focal length F and principal point CX, CY: the depth map goes to
// <out>-ray.pfm (0 where no surface is hit) and the normal map to <out>-ray-n.png in the encoding of --normals (byte = rint(127 * n) +
// 128 per component, made on the host; 0, 0, 0 where there is no normal); one line with the report's counts is printed.  STEP defaults
// to VOXEL / 2, SKIP to max(TRUNC / 2, STEP).  --view-pose FILE (only with --tsdf-raycast): the view's pose, a file like that of --pose;
// default: the pose of --pose.
// --tsdf-track MAP.pfm[,GUESS.txt] (only with --tsdf; refused otherwise while the arguments are parsed) tracks a second frame against the
// volume after the pair's map is fused (ADCensusStereo::TsdfTrack: the volume ray cast from the guess, then point-to-plane ICP on the
// device): MAP.pfm is a disparity map of the pair's size and calibration, GUESS.txt a file like that of --pose, default: the pose of
// --pose.  The parameters are the API's defaults with z_far = the distance from the guess camera to the volume's farthest corner.  One
// report line is printed and the recovered pose goes to <out>-track.txt, 12 numbers in the format --pose reads.
// --tsdf-fuse CW0,CW1,CW2,CW3,MINCONF,POWER,ZREF[,GAP] (only with --tsdf; refused otherwise while the arguments are parsed) fuses the map
// with ADCensusStereo::TsdfWeights / TsdfFuse instead of TsdfIntegrate: the provenance and confidence maps of the SAME Match become a
// weight per pixel (class weights CW0..CW3 of the four fill classes, pixels measured with a confidence below MINCONF get 0, the weight
// falls with (ZREF / Z)^POWER, POWER 0, 2 or 4) and, with GAP, the map is read by the bilinear interpolation gated by GAP disparities.
// --tsdf-mesh, --tsdf-raycast and --tsdf-track then see that volume; one more report line is printed; the run's other files are what
// they were.
// --tsdf-shift SX,SY,SZ[,MINW] (only with --tsdf; refused otherwise while the arguments are parsed) moves the volume's window by SX, SY, SZ
// voxels after the pair's map is fused (ADCensusStereo::TsdfShift) and writes the surface points whose voxels leave (weight >= MINW,
// default that of --tsdf) to <out>-tsdf-left.ply, a file like <out>-tsdf.ply; one more report line is printed.  <out>-tsdf.ply,
// --tsdf-mesh, --tsdf-raycast and --tsdf-track then see the shifted volume; the run's other files are what they are without the flag.
// --speckle SIZE,DIFF (anywhere after the program name) switches the device-side speckle filter on (ADCensusStereo::SetSpeckleFilter:
// components of at most SIZE pixels whose neighbours differ by at most DIFF become invalid): EVERY file of the run comes from
// the filtered map; without the flag the files are what they were.
// --rectify LEFT.txt,RIGHT.txt (anywhere after the program name) declares the two images RAW camera frames and rectifies them on the
// device in front of the Match (ADCensusStereo::SetRectifyModel).  Each file holds one camera as key=value lines ('#' starts a
// comment): width height pitch format (BGR8 RGB8 GRAY8 BGRA8: the layout the loaded pixels are repacked into before they are
// handed over) fx fy cx cy k1 k2 p1 p2 k3 R (nine values, row-major) new_fx new_fy new_cx new_cy, each exactly once, and optionally
// rect_width rect_height (the rectified size, default: the raw size; both files must agree).  A malformed flag or file is refused
// while the arguments are parsed.  Every file of the run then comes from the rectified pair, and the run also writes
//   <out>-rect-left.png  <out>-rect-right.png   the rectified images
// --raw FMT,W,H[,PITCH[,BITS]] (anywhere after the program name) declares the two image arguments headerless binary camera frames of
// that layout instead of image files: FMT one of BGR8 RGB8 GRAY8 BGRA8 GRAY16 BAYER_RGGB8 BAYER_GRBG8 BAYER_GBRG8 BAYER_BGGR8
// BAYER_RGGB16 BAYER_GRBG16 BAYER_GBRG16 BAYER_BGGR16 YUYV UYVY NV12, W x H the frame size, PITCH the bytes of a row (default:
// tightly packed), BITS the significant bits of a 16-bit layout (9..16, default 16).  Each file must hold exactly one frame.  Without
// --rectify the frames are already rectified and are only converted on the device (ADCensusStereo::SetInputFormat); with --rectify
// FMT,W,H,PITCH are the raw geometry of both cameras (the camera files' width and height must agree, their pitch and format are
// superseded).  A malformed flag is refused while the arguments are parsed.  The run also writes <out>-rect-left.png / -right.png.
// --register TARGET.txt[,COLOR.png] (anywhere after the program name; needs --calib) registers the depth of the run into a second
// camera on the device (ADCensusStereo::SetRegisterTarget / RegisterDepth).  TARGET.txt holds the numbers of adc_reg_target in
// declaration order, separated by white space: width height fx fy cx cy k1 k2 p1 p2 k3 R[0..8] t[0..2]; a malformed flag or file is
// refused while the arguments are parsed.  The run also writes <out>-reg.pfm (the registered depth, +inf where nothing landed); with a
// colour image of the target's size also <out>-aligned.png (the colour image aligned to the left view, ADCensusStereo::AlignColor),
// and the points of <out>-cloud.ply take their colours from it.
// --gt LEFT[,RIGHT],SCALE [--bad T0[,T1..]] (anywhere after the program name) scores the map against ground truth on the device
// (ADCensusStereo::SetGroundTruth / Evaluate): LEFT / RIGHT are the left- / right-view disparities as 8-bit gray PNG (0 = unknown) or
// PFM, disparity = value / SCALE (Middlebury: 4 for Cone, 2 for Cloth3 / Wood2, 1 for PFM); with RIGHT the non-occluded mask comes
// from the cross-check of the two.  --bad gives up to four thresholds (default 1).  A malformed flag is refused while the arguments
// are parsed.  With --extras the provenance and confidence maps are scored too (one row per fill class, the confidence's
// sparsification area); with --speckle the filtered map is what is scored.  Prints one table and writes
//   <out>-err.pfm    float32 |d - ground truth|, +inf where unknown or invalid
//   <out>-bad.png    the class map coloured: black unknown, blue invalid, grey good, red bad (darker / orange where occluded)
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ADCensusStereo.h"
#include "adcensus_c_api.h"
#include "adc_image_io.h"

struct RectifyFile { adc_raw_format raw; adc_camera_model model; int rect_w, rect_h; };

// one camera file of --rectify; false (with the reason in `why`) unless every key is there exactly once and every value parses
static bool parse_rectify_file(const std::string& path, RectifyFile& out, std::string& why)
{
    static const char* const keys[] = {"width", "height", "pitch", "format", "fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "R",
                                       "new_fx", "new_fy", "new_cx", "new_cy", "rect_width", "rect_height"};
    const int nkeys = 20, required = 18;
    int seen[20] = {0};
    FILE* f = fopen(path.c_str(), "r");
    if (!f) { why = "cannot read " + path; return false; }
    memset(&out, 0, sizeof(out));
    char line[1024];
    bool ok = true;
    while (ok && fgets(line, sizeof(line), f)) {
        std::string t(line);
        const size_t hash = t.find('#');
        if (hash != std::string::npos) t.resize(hash);
        while (!t.empty() && strchr(" \t\r\n", t.back())) t.pop_back();
        size_t b = 0;
        while (b < t.size() && (t[b] == ' ' || t[b] == '\t')) b++;
        t = t.substr(b);
        if (t.empty()) continue;
        const size_t eq = t.find('=');
        if (eq == std::string::npos) { why = path + ": not a key=value line: " + t; ok = false; break; }
        std::string key = t.substr(0, eq), val = t.substr(eq + 1);
        while (!key.empty() && (key.back() == ' ' || key.back() == '\t')) key.pop_back();
        int k = -1;
        for (int i = 0; i < nkeys; i++) if (key == keys[i]) k = i;
        if (k < 0) { why = path + ": unknown key " + key; ok = false; break; }
        if (seen[k]++) { why = path + ": key given twice: " + key; ok = false; break; }
        char tail = 0;
        if (k == 3) { // format: a name or its number
            while (!val.empty() && (val[0] == ' ' || val[0] == '\t')) val.erase(0, 1);
            static const char* const names[] = {"BGR8", "RGB8", "GRAY8", "BGRA8"};
            int fmt = -1;
            for (int i = 0; i < 4; i++) if (val == names[i] || (val.size() == 1 && val[0] == '0' + i)) fmt = i;
            if (fmt < 0) { why = path + ": format must be BGR8, RGB8, GRAY8 or BGRA8"; ok = false; break; }
            out.raw.format = fmt;
        } else if (k == 13) { // R: nine values
            for (char& c : val) if (c == ',') c = ' ';
            float* R = out.model.R;
            if (sscanf(val.c_str(), "%f %f %f %f %f %f %f %f %f %c", R, R + 1, R + 2, R + 3, R + 4, R + 5, R + 6, R + 7, R + 8, &tail) != 9) { why = path + ": R needs nine values"; ok = false; break; }
        } else if (k <= 2 || k >= 18) { // integers
            int v = 0;
            if (sscanf(val.c_str(), "%d %c", &v, &tail) != 1) { why = path + ": " + key + " needs an integer"; ok = false; break; }
            if (k == 0) out.raw.width = v; else if (k == 1) out.raw.height = v; else if (k == 2) out.raw.pitch_bytes = v; else if (k == 18) out.rect_w = v; else out.rect_h = v;
        } else { // floats
            float v = 0.f;
            if (sscanf(val.c_str(), "%f %c", &v, &tail) != 1) { why = path + ": " + key + " needs a number"; ok = false; break; }
            float* const dst[] = {&out.model.fx, &out.model.fy, &out.model.cx, &out.model.cy, &out.model.k1, &out.model.k2, &out.model.p1, &out.model.p2, &out.model.k3,
                                  nullptr, &out.model.new_fx, &out.model.new_fy, &out.model.new_cx, &out.model.new_cy};
            *dst[k - 4] = v;
        }
    }
    fclose(f);
    if (!ok) return false;
    for (int i = 0; i < required; i++) if (!seen[i]) { why = path + ": key missing: " + keys[i]; return false; }
    if (seen[18] != seen[19]) { why = path + ": rect_width and rect_height come together"; return false; }
    if (!seen[18]) { out.rect_w = out.raw.width; out.rect_h = out.raw.height; }
    const int bpp = out.raw.format == ADC_PIX_GRAY8 ? 1 : (out.raw.format == ADC_PIX_BGRA8 ? 4 : 3);
    if (out.raw.width < 1 || out.raw.width > 32767 || out.raw.height < 1 || out.raw.height > 32767 || (long long)out.raw.pitch_bytes < (long long)out.raw.width * bpp ||
        (long long)out.raw.height * out.raw.pitch_bytes > 2147483647LL || out.rect_w < 1 || out.rect_h < 1) { why = path + ": width / height / pitch out of range"; return false; }
    const float* v = &out.model.fx;
    for (size_t i = 0; i < sizeof(adc_camera_model) / sizeof(float); i++) if (!std::isfinite(v[i])) { why = path + ": every value must be finite"; return false; }
    if (out.model.fx == 0.f || out.model.fy == 0.f || out.model.new_fx == 0.f || out.model.new_fy == 0.f) { why = path + ": fx, fy, new_fx, new_fy must not be 0"; return false; }
    return true;
}

static long long raw_frame_bytes(const adc_raw_format& f)
{
    const long long luma = (long long)f.height * f.pitch_bytes;
    return (f.format & 0xff) == ADC_PIX_NV12 ? luma / 2 * 3 : luma;
}

// the value of --raw; false (with the reason in `why`) unless it names a layout and a geometry the library accepts
static bool parse_raw_flag(const std::string& v, adc_raw_format& out, std::string& why)
{
    static const struct { const char* name; int code, bpp; } layouts[] = {
        {"BGR8", ADC_PIX_BGR8, 3}, {"RGB8", ADC_PIX_RGB8, 3}, {"GRAY8", ADC_PIX_GRAY8, 1}, {"BGRA8", ADC_PIX_BGRA8, 4}, {"GRAY16", ADC_PIX_GRAY16, 2},
        {"BAYER_RGGB8", ADC_PIX_BAYER_RGGB8, 1}, {"BAYER_GRBG8", ADC_PIX_BAYER_GRBG8, 1}, {"BAYER_GBRG8", ADC_PIX_BAYER_GBRG8, 1}, {"BAYER_BGGR8", ADC_PIX_BAYER_BGGR8, 1},
        {"BAYER_RGGB16", ADC_PIX_BAYER_RGGB16, 2}, {"BAYER_GRBG16", ADC_PIX_BAYER_GRBG16, 2}, {"BAYER_GBRG16", ADC_PIX_BAYER_GBRG16, 2}, {"BAYER_BGGR16", ADC_PIX_BAYER_BGGR16, 2},
        {"YUYV", ADC_PIX_YUYV, 2}, {"UYVY", ADC_PIX_UYVY, 2}, {"NV12", ADC_PIX_NV12, 1}};
    std::vector<std::string> parts;
    size_t at = 0, comma;
    while ((comma = v.find(',', at)) != std::string::npos) { parts.push_back(v.substr(at, comma - at)); at = comma + 1; }
    parts.push_back(v.substr(at));
    why = "it needs FMT,W,H[,PITCH[,BITS]]";
    if (parts.size() < 3 || parts.size() > 5) return false;
    int code = -1, bpp = 0;
    for (const auto& l : layouts) if (parts[0] == l.name) { code = l.code; bpp = l.bpp; }
    if (code < 0) { why = "unknown layout " + parts[0]; return false; }
    int n[4] = {0, 0, 0, 0}; // W, H, PITCH, BITS
    for (size_t i = 1; i < parts.size(); i++) {
        char tail = 0;
        if (sscanf(parts[i].c_str(), "%d%c", &n[i - 1], &tail) != 1 || n[i - 1] < 0) { why = "not a number: " + parts[i]; return false; }
    }
    const bool wide = bpp == 2 && code != ADC_PIX_YUYV && code != ADC_PIX_UYVY, yuv = code == ADC_PIX_YUYV || code == ADC_PIX_UYVY || code == ADC_PIX_NV12;
    const bool bayer = code >= ADC_PIX_BAYER_RGGB8 && code <= ADC_PIX_BAYER_BGGR16;
    if (n[0] < 1 || n[0] > 32767 || n[1] < 1 || n[1] > 32767) { why = "W and H must be 1..32767"; return false; }
    if (parts.size() < 4 || n[2] == 0) n[2] = n[0] * bpp;
    if (n[2] < n[0] * bpp) { why = "PITCH is smaller than a row"; return false; }
    if (n[3] != 0 && !(wide && n[3] >= 9 && n[3] <= 16)) { why = "BITS must be 9..16 and belongs to a 16-bit layout"; return false; }
    if (wide && (n[2] & 1)) { why = "PITCH of a 16-bit layout must be even"; return false; }
    if (bayer && (n[0] < 2 || n[1] < 2)) { why = "a Bayer frame needs W and H >= 2"; return false; }
    if ((yuv && (n[0] & 1)) || (code == ADC_PIX_NV12 && (n[1] & 1))) { why = "W (NV12: and H) of a YUV layout must be even"; return false; }
    out.width = n[0]; out.height = n[1]; out.pitch_bytes = n[2]; out.format = ADC_PIX_BITS(code, n[3]);
    if (raw_frame_bytes(out) > 2147483647LL) { why = "a frame must be smaller than 2 GiB"; return false; }
    return true;
}

// one headerless frame: the file must hold exactly the declared bytes
static bool load_raw_frame(const char* path, const adc_raw_format& f, std::vector<uint8>& out)
{
    FILE* fp = fopen(path, "rb");
    if (!fp) return false;
    const size_t n = (size_t)raw_frame_bytes(f);
    out.assign(n, 0);
    uint8 extra = 0;
    const bool ok = fread(out.data(), 1, n, fp) == n && fread(&extra, 1, 1, fp) == 0;
    fclose(fp);
    return ok;
}

// tightly packed B,G,R pixels -> the declared raw layout (GRAY8 takes B; alpha and row padding are 0)
static std::vector<uint8> pack_raw(const std::vector<uint8>& bgr, const adc_raw_format& f)
{
    std::vector<uint8> raw((size_t)f.height * f.pitch_bytes, 0);
    for (int y = 0; y < f.height; y++)
        for (int x = 0; x < f.width; x++) {
            const uint8* p = &bgr[((size_t)y * f.width + x) * 3];
            uint8* q = &raw[(size_t)y * f.pitch_bytes];
            if (f.format == ADC_PIX_GRAY8) q[x] = p[0];
            else if (f.format == ADC_PIX_RGB8) { q[3 * x] = p[2]; q[3 * x + 1] = p[1]; q[3 * x + 2] = p[0]; }
            else if (f.format == ADC_PIX_BGRA8) { q[4 * x] = p[0]; q[4 * x + 1] = p[1]; q[4 * x + 2] = p[2]; }
            else { q[3 * x] = p[0]; q[3 * x + 1] = p[1]; q[3 * x + 2] = p[2]; }
        }
    return raw;
}

// PFM ("Pf", one channel) -> rows top-down; false unless the header and the payload are complete
static bool load_pfm(const std::string& path, std::vector<float32>& px, int& w, int& h)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char magic[3] = {0};
    float scale = 0.f;
    bool ok = fscanf(f, "%2s %d %d %f", magic, &w, &h, &scale) == 4 && !strcmp(magic, "Pf") && w > 0 && h > 0 && (long long)w * h <= (1LL << 30) && fgetc(f) != EOF;
    if (ok) {
        px.resize((size_t)w * h);
        for (int y = h - 1; ok && y >= 0; y--) ok = fread(&px[(size_t)y * w], 4, (size_t)w, f) == (size_t)w;
        if (ok && scale > 0.f) // big-endian payload
            for (float32& v : px) { uint8 b[4]; memcpy(b, &v, 4); const uint8 r[4] = {b[3], b[2], b[1], b[0]}; memcpy(&v, r, 4); }
    }
    fclose(f);
    return ok;
}

// one view's ground truth from an 8-bit gray PNG or a PFM of w x h pixels
struct GtImage { std::vector<uint8> u8; std::vector<float32> f32; adc_gt gt; };
static bool load_gt(const std::string& path, float scale, int w, int h, GtImage& out, std::string& why)
{
    int gw = 0, gh = 0;
    memset(&out.gt, 0, sizeof(out.gt));
    out.gt.scale = scale;
    if (path.size() > 4 && path.substr(path.size() - 4) == ".pfm") {
        if (!load_pfm(path, out.f32, gw, gh)) { why = "cannot read " + path + " (one-channel PFM)"; return false; }
        out.gt.data = out.f32.data();
        out.gt.format = ADC_GT_F32;
    } else {
        std::vector<uint8> bgr;
        if (!load_image(path.c_str(), bgr, gw, gh)) { why = "cannot read " + path + " (8-bit gray PNG or PFM)"; return false; }
        out.u8.resize((size_t)gw * gh);
        for (size_t i = 0; i < out.u8.size(); i++) {
            if (bgr[3 * i] != bgr[3 * i + 1] || bgr[3 * i] != bgr[3 * i + 2]) { why = path + " is not a gray image"; return false; }
            out.u8[i] = bgr[3 * i];
        }
        out.gt.data = out.u8.data();
        out.gt.format = ADC_GT_U8;
    }
    if (gw != w || gh != h) { why = path + " does not have the size of the images"; return false; }
    return true;
}

static void print_eval_row(const char* name, uint64_t pixels, uint64_t invalid, const uint64_t* bad, int n, uint64_t sum_q, const uint64_t* sum_sq_q)
{
    const double valid = (double)(pixels - invalid);
    printf("%-14s %9llu %8.2f", name, (unsigned long long)pixels, pixels ? 100.0 * (double)invalid / (double)pixels : 0.0);
    for (int k = 0; k < n; k++) printf(" %9.2f", pixels ? 100.0 * (double)bad[k] / (double)pixels : 0.0);
    printf(" %8.4f", valid > 0 ? (double)sum_q / 1024.0 / valid : 0.0);
    if (sum_sq_q) printf(" %8.4f", valid > 0 ? sqrt((double)*sum_sq_q / (1024.0 * 1024.0) / valid) : 0.0);
    printf("\n");
}

// the file of --register; false (with the reason in `why`) unless it holds exactly the numbers of adc_reg_target, all usable
static bool parse_register_file(const std::string& path, adc_reg_target& out, std::string& why)
{
    FILE* f = fopen(path.c_str(), "r");
    if (!f) { why = "cannot read " + path; return false; }
    double v[23];
    int n = 0;
    while (n < 23 && fscanf(f, "%lf", &v[n]) == 1) n++;
    char tail[2];
    const bool more = fscanf(f, "%1s", tail) == 1;
    fclose(f);
    if (n != 23 || more) { why = path + ": it holds width height fx fy cx cy k1 k2 p1 p2 k3, nine numbers of R and three of t, nothing else"; return false; }
    for (int i = 0; i < 23; i++)
        if (!std::isfinite(v[i]) || !std::isfinite((float)v[i])) { why = path + ": a value is not finite"; return false; }
    if (v[0] != std::floor(v[0]) || v[1] != std::floor(v[1]) || v[0] < 1 || v[0] > 32767 || v[1] < 1 || v[1] > 32767) {
        why = path + ": width and height must be whole numbers in [1, 32767]";
        return false;
    }
    if ((float)v[2] == 0.f || (float)v[3] == 0.f) { why = path + ": fx and fy must not be 0"; return false; }
    out.width = (int32_t)v[0]; out.height = (int32_t)v[1];
    out.fx = (float)v[2]; out.fy = (float)v[3]; out.cx = (float)v[4]; out.cy = (float)v[5];
    out.k1 = (float)v[6]; out.k2 = (float)v[7]; out.p1 = (float)v[8]; out.p2 = (float)v[9]; out.k3 = (float)v[10];
    for (int i = 0; i < 9; i++) out.R[i] = (float)v[11 + i];
    for (int i = 0; i < 3; i++) out.t[i] = (float)v[20 + i];
    return true;
}

static void write_pfm(const std::string& path, const float32* px, int w, int h)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (f) { fprintf(f, "Pf\n%d %d\n-1.0\n", w, h); for (int y = h - 1; y >= 0; y--) fwrite(&px[(size_t)y * w], 4, w, f); fclose(f); }
}

int main(int argc, char** argv)
{
    bool extras = false; // (--extras is taken out of argv: the positional arguments keep their meaning)
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--extras")) {
            extras = true;
            for (int j = i; j + 1 < argc; j++) argv[j] = argv[j + 1];
            argc--;
            break;
        }
    bool with_calib = false; // (--calib and its value are taken out of argv in the same way)
    adc_calib calib = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--calib")) {
            if (i + 1 >= argc || sscanf(argv[i + 1], "%f,%f,%f,%f,%f", &calib.focal_px, &calib.baseline, &calib.cx, &calib.cy, &calib.doffs) != 5) {
                printf("--calib needs f,B,cx,cy,doffs\n");
                return -1;
            }
            with_calib = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    int speckle_size = 0; // (--speckle and its value likewise; checked before anything touches a device)
    float speckle_diff = 0.f;
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--speckle")) {
            char tail = 0;
            if (i + 1 >= argc || sscanf(argv[i + 1], "%d,%f%c", &speckle_size, &speckle_diff, &tail) != 2 || speckle_size <= 0 ||
                !std::isfinite(speckle_diff) || speckle_diff < 0.f) {
                printf("--speckle needs SIZE,DIFF (SIZE > 0 pixels, DIFF >= 0 and finite)\n");
                return -1;
            }
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    bool with_voxel = false; // (--voxel and its value likewise; checked before anything touches a device)
    adc_voxel_grid voxel_grid;
    memset(&voxel_grid, 0, sizeof(voxel_grid));
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--voxel")) {
            char tail = 0;
            voxel_grid.z_min = 0.f;
            voxel_grid.z_max = INFINITY;
            int n = i + 1 < argc ? sscanf(argv[i + 1], "%f,%f,%f%c", &voxel_grid.leaf, &voxel_grid.z_min, &voxel_grid.z_max, &tail) : 0;
            if (n == 1 && sscanf(argv[i + 1], "%f%c", &voxel_grid.leaf, &tail) != 1) n = 0; // (LEAF alone: nothing may follow it)
            if ((n != 1 && n != 3) || !std::isfinite(voxel_grid.leaf) || voxel_grid.leaf <= 0.f ||
                !(voxel_grid.z_min <= voxel_grid.z_max)) {
                printf("--voxel needs LEAF[,ZMIN,ZMAX] (LEAF > 0 and finite, ZMIN <= ZMAX)\n");
                return -1;
            }
            with_voxel = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    if (with_voxel && !with_calib) { printf("--voxel refused: it needs --calib\n"); return -1; }
    bool with_normals = false; // (--normals and its value likewise; checked before anything touches a device)
    adc_normals_params normals_params;
    memset(&normals_params, 0, sizeof(normals_params));
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--normals")) {
            char tail = 0;
            normals_params.max_diff = 1.0f;
            normals_params.min_points = 5;
            const char* v = i + 1 < argc ? argv[i + 1] : "";
            int n = sscanf(v, "%d,%f,%d%c", &normals_params.radius, &normals_params.max_diff, &normals_params.min_points, &tail);
            if (n == 1 && sscanf(v, "%d%c", &normals_params.radius, &tail) != 1) n = 0; // (R alone: nothing may follow it)
            if (n == 2 && sscanf(v, "%d,%f%c", &normals_params.radius, &normals_params.max_diff, &tail) != 2) n = 0;
            const int side = (n >= 1 && normals_params.radius >= 1 && normals_params.radius <= ADC_NORMALS_MAX_RADIUS) ? 2 * normals_params.radius + 1 : 0;
            if (n < 1 || n > 3 || side == 0 || !std::isfinite(normals_params.max_diff) || !(normals_params.max_diff > 0.f && normals_params.max_diff <= 64.f) ||
                normals_params.min_points < 3 || normals_params.min_points > side * side) {
                printf("--normals refused: it needs R[,DIFF[,MIN]] (R in 1..7, 0 < DIFF <= 64, 3 <= MIN <= (2R+1)^2)\n");
                return -1;
            }
            with_normals = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= i + 1 < argc ? 2 : 1;
            break;
        }
    if (with_normals && !with_calib) { printf("--normals refused: it needs --calib\n"); return -1; }
    bool with_mesh = false; // (--mesh and its value likewise; checked before anything touches a device)
    adc_mesh_params mesh_params;
    memset(&mesh_params, 0, sizeof(mesh_params));
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--mesh")) {
            char tail = 0;
            mesh_params.step = 1;
            const char* v = i + 1 < argc ? argv[i + 1] : "";
            int n = sscanf(v, "%f,%d%c", &mesh_params.max_diff, &mesh_params.step, &tail);
            if (n == 1 && sscanf(v, "%f%c", &mesh_params.max_diff, &tail) != 1) n = 0; // (DIFF alone: nothing may follow it)
            if (n < 1 || n > 2 || !(mesh_params.max_diff >= 0.f) || mesh_params.step < 1 || mesh_params.step > ADC_MESH_MAX_STEP) {
                printf("--mesh refused: it needs DIFF[,STEP] (DIFF >= 0 or inf, STEP in 1..16)\n");
                return -1;
            }
            with_mesh = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= i + 1 < argc ? 2 : 1;
            break;
        }
    bool with_tsdf = false, with_pose = false; // (--tsdf, --pose and their values likewise; the pose file is read and checked here)
    adc_tsdf_params tsdf_params;
    adc_tsdf_extract_params tsdf_extract;
    adc_tsdf_frame tsdf_frame;
    memset(&tsdf_params, 0, sizeof(tsdf_params));
    memset(&tsdf_extract, 0, sizeof(tsdf_extract));
    memset(&tsdf_frame, 0, sizeof(tsdf_frame));
    tsdf_frame.R[0] = tsdf_frame.R[4] = tsdf_frame.R[8] = 1.0f;
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--tsdf")) {
            char tail = 0;
            adc_tsdf_params& t = tsdf_params;
            const char* v = i + 1 < argc ? argv[i + 1] : "";
            int minw = 1;
            int n = sscanf(v, "%d,%d,%d,%f,%f,%f,%f,%f,%d%c", &t.nx, &t.ny, &t.nz, &t.voxel, &t.origin[0], &t.origin[1], &t.origin[2], &t.trunc, &minw, &tail);
            if (n == 7 && sscanf(v, "%d,%d,%d,%f,%f,%f,%f%c", &t.nx, &t.ny, &t.nz, &t.voxel, &t.origin[0], &t.origin[1], &t.origin[2], &tail) != 7) n = 0;
            if (n == 8 && sscanf(v, "%d,%d,%d,%f,%f,%f,%f,%f%c", &t.nx, &t.ny, &t.nz, &t.voxel, &t.origin[0], &t.origin[1], &t.origin[2], &t.trunc, &tail) != 8) n = 0;
            if (n == 7) t.trunc = 3.0f * t.voxel;
            t.z_min = 0.0f;
            t.z_max = INFINITY;
            t.max_weight = 64;
            t.flags = ADC_TSDF_COLOR;
            const bool dims = n >= 7 && n <= 9 && t.nx >= 4 && t.ny >= 4 && t.nz >= 4 && t.nx <= ADC_TSDF_MAX_DIM && t.ny <= ADC_TSDF_MAX_DIM && t.nz <= ADC_TSDF_MAX_DIM &&
                              t.nx % 4 == 0 && (unsigned long long)t.nx * t.ny * t.nz <= (1ull << 30);
            if (!dims || !(std::isfinite(t.voxel) && t.voxel > 0.f) || !std::isfinite(t.origin[0]) || !std::isfinite(t.origin[1]) || !std::isfinite(t.origin[2]) ||
                !(std::isfinite(t.trunc) && t.trunc > 0.f) || minw < 1 || minw > 65535) {
                printf("--tsdf refused: it needs NX,NY,NZ,VOXEL,OX,OY,OZ[,TRUNC[,MINW]] (sizes in 4..2048, NX a multiple of 4, at most 2^30 voxels, VOXEL > 0, TRUNC > 0, MINW in 1..65535)\n");
                return -1;
            }
            tsdf_extract.min_weight = (uint32)minw;
            with_tsdf = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= i + 1 < argc ? 2 : 1;
            break;
        }
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--pose")) {
            FILE* f = i + 1 < argc ? fopen(argv[i + 1], "r") : nullptr;
            float v[12];
            int n = 0;
            char extra = 0;
            while (f && n < 12 && fscanf(f, "%f", &v[n]) == 1 && std::isfinite(v[n])) n++;
            const bool clean = f && n == 12 && fscanf(f, " %c", &extra) != 1;
            if (f) fclose(f);
            if (!clean) { printf("--pose refused: it needs a file of 12 finite numbers (R row-major, then t)\n"); return -1; }
            for (int k = 0; k < 9; k++) tsdf_frame.R[k] = v[k];
            for (int k = 0; k < 3; k++) tsdf_frame.t[k] = v[9 + k];
            with_pose = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    bool with_tsdf_mesh = false; // (--tsdf-mesh, no value)
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--tsdf-mesh")) {
            with_tsdf_mesh = true;
            for (int j = i; j + 1 < argc; j++) argv[j] = argv[j + 1];
            argc -= 1;
            break;
        }
    bool with_tsdf_raycast = false, with_view_pose = false; // (--tsdf-raycast, --view-pose and their values likewise)
    adc_tsdf_raycast_params ray_view;
    memset(&ray_view, 0, sizeof(ray_view));
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--tsdf-raycast")) {
            char tail = 0;
            adc_tsdf_raycast_params& r = ray_view;
            const char* v = i + 1 < argc ? argv[i + 1] : "";
            int n = sscanf(v, "%d,%d,%f,%f,%f,%f,%f%c", &r.width, &r.height, &r.focal_px, &r.cx, &r.cy, &r.step, &r.skip, &tail);
            if (n == 5 && sscanf(v, "%d,%d,%f,%f,%f%c", &r.width, &r.height, &r.focal_px, &r.cx, &r.cy, &tail) != 5) n = 0;
            if (n == 6 && sscanf(v, "%d,%d,%f,%f,%f,%f%c", &r.width, &r.height, &r.focal_px, &r.cx, &r.cy, &r.step, &tail) != 6) n = 0;
            if (n < 6) r.step = 0.0f; // (0: filled in from the volume below)
            if (n < 7) r.skip = 0.0f;
            if (n < 5 || n > 7 || r.width < 1 || r.height < 1 || r.width > 8192 || r.height > 8192 || !(std::isfinite(r.focal_px) && r.focal_px > 0.f) ||
                !std::isfinite(r.cx) || !std::isfinite(r.cy) || (n >= 6 && !(std::isfinite(r.step) && r.step > 0.f)) ||
                (n == 7 && !(std::isfinite(r.skip) && r.skip >= r.step))) {
                printf("--tsdf-raycast refused: it needs W,H,F,CX,CY[,STEP[,SKIP]] (W, H in 1..8192, F > 0, STEP > 0, SKIP >= STEP)\n");
                return -1;
            }
            with_tsdf_raycast = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= i + 1 < argc ? 2 : 1;
            break;
        }
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--view-pose")) {
            if (!with_tsdf_raycast) { printf("--view-pose refused: it needs --tsdf-raycast\n"); return -1; }
            if (!with_tsdf) break; // (refused below, before the file is looked at)
            FILE* f = i + 1 < argc ? fopen(argv[i + 1], "r") : nullptr;
            float v[12];
            int n = 0;
            char extra = 0;
            while (f && n < 12 && fscanf(f, "%f", &v[n]) == 1 && std::isfinite(v[n])) n++;
            const bool clean = f && n == 12 && fscanf(f, " %c", &extra) != 1;
            if (f) fclose(f);
            if (!clean) { printf("--view-pose refused: it needs a file of 12 finite numbers (R row-major, then t)\n"); return -1; }
            for (int k = 0; k < 9; k++) ray_view.R[k] = v[k];
            for (int k = 0; k < 3; k++) ray_view.t[k] = v[9 + k];
            with_view_pose = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    bool with_tsdf_track = false, with_track_guess = false; // (--tsdf-track and its value likewise; the guess file is read and checked here)
    std::string track_map;
    float track_guess[12];
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--tsdf-track")) {
            if (!with_tsdf) { printf("--tsdf-track refused: it needs --tsdf\n"); return -1; }
            const std::string v = i + 1 < argc ? argv[i + 1] : "";
            const size_t comma = v.find(',');
            track_map = v.substr(0, comma);
            if (track_map.empty()) { printf("--tsdf-track refused: it needs MAP.pfm[,GUESS.txt]\n"); return -1; }
            if (comma != std::string::npos) {
                FILE* f = fopen(v.substr(comma + 1).c_str(), "r");
                int n = 0;
                char extra = 0;
                while (f && n < 12 && fscanf(f, "%f", &track_guess[n]) == 1 && std::isfinite(track_guess[n])) n++;
                const bool clean = f && n == 12 && fscanf(f, " %c", &extra) != 1;
                if (f) fclose(f);
                if (!clean) { printf("--tsdf-track refused: the guess needs a file of 12 finite numbers (R row-major, then t)\n"); return -1; }
                with_track_guess = true;
            }
            with_tsdf_track = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= i + 1 < argc ? 2 : 1;
            break;
        }
    bool with_tsdf_fuse = false; // (--tsdf-fuse and its value likewise)
    adc_tsdf_weight_params fuse_weights;
    adc_tsdf_fuse_params fuse_params;
    memset(&fuse_weights, 0, sizeof(fuse_weights));
    memset(&fuse_params, 0, sizeof(fuse_params));
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--tsdf-fuse")) {
            if (!with_tsdf) { printf("--tsdf-fuse refused: it needs --tsdf\n"); return -1; }
            const char* v = i + 1 < argc ? argv[i + 1] : "";
            int cw[4] = {-1, -1, -1, -1}, power = -1;
            float minconf = -1.0f, zref = 0.0f, gap = -1.0f;
            char tail = 0;
            int n = sscanf(v, "%d,%d,%d,%d,%f,%d,%f,%f%c", &cw[0], &cw[1], &cw[2], &cw[3], &minconf, &power, &zref, &gap, &tail);
            if (n == 7 && sscanf(v, "%d,%d,%d,%d,%f,%d,%f%c", &cw[0], &cw[1], &cw[2], &cw[3], &minconf, &power, &zref, &tail) != 7) n = 0;
            bool fine = (n == 7 || n == 8) && minconf >= 0.0f && minconf <= 1.0f && (power == 0 || power == 2 || power == 4) && std::isfinite(zref) && zref > 0.0f &&
                        (n == 7 || (std::isfinite(gap) && gap >= 0.0f));
            for (int k = 0; k < 4; k++) fine = fine && cw[k] >= 0 && cw[k] <= 255;
            if (!fine) {
                printf("--tsdf-fuse refused: it needs CW0,CW1,CW2,CW3,MINCONF,POWER,ZREF[,GAP] (CW in 0..255, MINCONF in 0..1, POWER 0, 2 or 4, ZREF > 0, GAP >= 0)\n");
                return -1;
            }
            for (int k = 0; k < 4; k++) fuse_weights.class_weight[k] = (uint8)cw[k];
            fuse_weights.min_confidence = minconf;
            fuse_weights.depth_power = (uint32)power;
            fuse_weights.z_ref = zref;
            if (n == 8) { fuse_params.flags = ADC_TSDF_FUSE_BILINEAR; fuse_params.interp_gap = gap; }
            with_tsdf_fuse = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= i + 1 < argc ? 2 : 1;
            break;
        }
    bool with_tsdf_shift = false; // (--tsdf-shift and its value likewise)
    adc_tsdf_shift_params tsdf_shift;
    memset(&tsdf_shift, 0, sizeof(tsdf_shift));
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--tsdf-shift")) {
            if (!with_tsdf) { printf("--tsdf-shift refused: it needs --tsdf\n"); return -1; }
            const char* v = i + 1 < argc ? argv[i + 1] : "";
            int s[3] = {0, 0, 0}, minw = (int)tsdf_extract.min_weight;
            char tail = 0;
            int n = sscanf(v, "%d,%d,%d,%d%c", &s[0], &s[1], &s[2], &minw, &tail);
            if (n == 3 && sscanf(v, "%d,%d,%d%c", &s[0], &s[1], &s[2], &tail) != 3) n = 0;
            bool fine = (n == 3 || n == 4) && minw >= 1 && minw <= 65535;
            for (int k = 0; k < 3; k++) fine = fine && s[k] >= -(1 << 24) && s[k] <= (1 << 24);
            if (!fine) {
                printf("--tsdf-shift refused: it needs SX,SY,SZ[,MINW] (whole voxels, each at most 2^24 in size, MINW in 1..65535)\n");
                return -1;
            }
            for (int k = 0; k < 3; k++) tsdf_shift.shift[k] = s[k];
            tsdf_shift.min_weight = (uint32)minw;
            with_tsdf_shift = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= i + 1 < argc ? 2 : 1;
            break;
        }
    if (with_tsdf_raycast && !with_tsdf) { printf("--tsdf-raycast refused: it needs --tsdf\n"); return -1; }
    if (with_tsdf_mesh && !with_tsdf) { printf("--tsdf-mesh refused: it needs --tsdf\n"); return -1; }
    if (with_tsdf && !with_calib) { printf("--tsdf refused: it needs --calib\n"); return -1; }
    if (with_pose && !with_tsdf) { printf("--pose refused: it needs --tsdf\n"); return -1; }
    bool with_rectify = false; // (--rectify and its value likewise; both files are read and checked here)
    RectifyFile rect_file[2];
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--rectify")) {
            std::string why = "--rectify needs LEFT.txt,RIGHT.txt";
            bool ok = i + 1 < argc;
            if (ok) {
                const std::string v(argv[i + 1]);
                const size_t comma = v.find(',');
                ok = comma != std::string::npos && comma > 0 && comma + 1 < v.size() && v.find(',', comma + 1) == std::string::npos;
                ok = ok && parse_rectify_file(v.substr(0, comma), rect_file[0], why) && parse_rectify_file(v.substr(comma + 1), rect_file[1], why);
                if (ok && (rect_file[0].rect_w != rect_file[1].rect_w || rect_file[0].rect_h != rect_file[1].rect_h)) { ok = false; why = "the two files differ in the rectified size"; }
            }
            if (!ok) { printf("--rectify refused: %s\n", why.c_str()); return -1; }
            with_rectify = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    bool with_raw = false; // (--raw and its value likewise)
    adc_raw_format raw_fmt = {0, 0, 0, 0};
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--raw")) {
            std::string why = "it needs FMT,W,H[,PITCH[,BITS]]";
            bool ok = i + 1 < argc && parse_raw_flag(argv[i + 1], raw_fmt, why);
            if (ok && with_rectify && (rect_file[0].raw.width != raw_fmt.width || rect_file[0].raw.height != raw_fmt.height ||
                                       rect_file[1].raw.width != raw_fmt.width || rect_file[1].raw.height != raw_fmt.height)) {
                ok = false; why = "W x H is not the raw size of the camera files of --rectify";
            }
            if (!ok) { printf("--raw refused: %s\n", why.c_str()); return -1; }
            with_raw = true;
            if (with_rectify) rect_file[0].raw = rect_file[1].raw = raw_fmt;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    bool with_gt = false; // (--gt / --bad and their values likewise; the syntax is checked here, the files are read behind the images)
    std::string gt_path[2];
    float gt_scale = 0.f;
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--gt")) {
            bool ok = i + 1 < argc;
            if (ok) {
                std::vector<std::string> parts;
                std::string v(argv[i + 1]);
                size_t at = 0, comma;
                while ((comma = v.find(',', at)) != std::string::npos) { parts.push_back(v.substr(at, comma - at)); at = comma + 1; }
                parts.push_back(v.substr(at));
                char tail = 0;
                ok = (parts.size() == 2 || parts.size() == 3) && !parts[0].empty() && (parts.size() == 2 || !parts[1].empty()) &&
                     sscanf(parts.back().c_str(), "%f%c", &gt_scale, &tail) == 1 && std::isfinite(gt_scale) && gt_scale > 0.f;
                if (ok) { gt_path[0] = parts[0]; if (parts.size() == 3) gt_path[1] = parts[1]; }
            }
            if (!ok) { printf("--gt refused: it needs LEFT[,RIGHT],SCALE (8-bit gray PNG or PFM; SCALE finite and > 0)\n"); return -1; }
            with_gt = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    adc_eval_params eval_params = {1, {1.0f, 0.f, 0.f, 0.f}};
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--bad")) {
            bool ok = i + 1 < argc && with_gt;
            int n = 0;
            if (ok) {
                const char* p = argv[i + 1];
                while (ok) {
                    char* end = nullptr;
                    const float t = strtof(p, &end);
                    ok = end != p && n < ADC_EVAL_MAX_THRESHOLDS && std::isfinite(t) && t >= 0.f && (*end == ',' || *end == 0);
                    if (!ok) break;
                    eval_params.thresholds[n++] = t;
                    if (*end == 0) break;
                    p = end + 1;
                }
            }
            if (!ok) { printf("--bad refused: it needs --gt and T0[,T1..] (one to four thresholds, finite and >= 0)\n"); return -1; }
            eval_params.n_thresholds = n;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    bool with_disp16 = false; // (--disp16 and its value likewise)
    float disp16_scale = 0.f;
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--disp16")) {
            char tail = 0;
            if (i + 1 >= argc || sscanf(argv[i + 1], "%f%c", &disp16_scale, &tail) != 1 || !std::isfinite(disp16_scale) || disp16_scale <= 0.f) {
                printf("--disp16 needs SCALE (finite and > 0; 256 is KITTI's encoding)\n");
                return -1;
            }
            with_disp16 = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    bool with_register = false; // (--register and its value likewise; the target file is read and checked here, the colour image behind the pair)
    adc_reg_target reg_target;
    std::string reg_color;
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "--register")) {
            std::string why = "it needs TARGET.txt[,COLOR.png]";
            bool ok = i + 1 < argc;
            if (ok) {
                const std::string v(argv[i + 1]);
                const size_t comma = v.find(',');
                const std::string file = v.substr(0, comma);
                if (comma != std::string::npos) reg_color = v.substr(comma + 1);
                ok = !file.empty() && (comma == std::string::npos || (!reg_color.empty() && reg_color.find(',') == std::string::npos));
                ok = ok && parse_register_file(file, reg_target, why);
            }
            if (!ok) { printf("--register refused: %s\n", why.c_str()); return -1; }
            with_register = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    if (with_register && !with_calib) { printf("--register refused: it needs --calib\n"); return -1; }
    if (with_calib && with_gt) { printf("--calib and --gt are separate runs\n"); return -1; }
    if (with_calib && extras) { printf("--calib and --extras are separate runs\n"); return -1; }
    // file-format helpers that need no GPU (used by the CPU test tier):
    //   --convert in.{png,ppm} out.png       decode + re-encode (R,G,B)
    //   --colormap in-d.png out-c.png        the JET mapping SaveDisparityMap applies to the grey disparity image
    if (argc == 4 && (!strcmp(argv[1], "--convert") || !strcmp(argv[1], "--colormap"))) {
        std::vector<uint8> bgr;
        int cw = 0, chh = 0;
        if (!load_image(argv[2], bgr, cw, chh)) { printf("cannot read %s\n", argv[2]); return -1; }
        std::vector<uint8> rgb(bgr.size());
        for (size_t i = 0; i < (size_t)cw * chh; i++) {
            if (!strcmp(argv[1], "--convert")) { rgb[3 * i] = bgr[3 * i + 2]; rgb[3 * i + 1] = bgr[3 * i + 1]; rgb[3 * i + 2] = bgr[3 * i]; }
            else { const uint8 g = bgr[3 * i + 1]; rgb[3 * i] = kJet[g][0]; rgb[3 * i + 1] = kJet[g][1]; rgb[3 * i + 2] = kJet[g][2]; }
        }
        return write_png(argv[3], rgb.data(), cw, chh, 3) ? 0 : -1;
    }
    if (argc < 3) {
        printf("usage: %s left.png right.png [min_disparity] [max_disparity] [out_prefix]\n", argv[0]);
        return -1;
    }
    printf("Image Loading...");
    std::vector<uint8> left, right;
    int w = 0, h = 0, w2 = 0, h2 = 0;
    if (with_raw) {
        if (!load_raw_frame(argv[1], raw_fmt, left) || !load_raw_frame(argv[2], raw_fmt, right)) {
            printf("cannot read the frame pair (--raw: each file holds exactly one frame of %lld bytes)\n", raw_frame_bytes(raw_fmt));
            return -1;
        }
        w = w2 = raw_fmt.width;
        h = h2 = raw_fmt.height;
    } else if (!load_image(argv[1], left, w, h) || !load_image(argv[2], right, w2, h2)) {
        printf("cannot read the image pair (8-bit PNG or binary PPM)\n"); // main.cpp:50-53
        return -1;
    }
    if (!with_rectify && (w != w2 || h != h2)) {
        printf("the two images differ in size\n"); // main.cpp:54-57
        return -1;
    }
    if (with_rectify) { // the loaded pixels become the raw frames of the declared layout; from here on w x h is the rectified size
        if (w != rect_file[0].raw.width || h != rect_file[0].raw.height || w2 != rect_file[1].raw.width || h2 != rect_file[1].raw.height) {
            printf("--rectify: an image does not have the size its camera file declares\n");
            return -1;
        }
        if (!with_raw) { // (--raw: the files are the frames already)
            left = pack_raw(left, rect_file[0].raw);
            right = pack_raw(right, rect_file[1].raw);
        }
        w = rect_file[0].rect_w;
        h = rect_file[0].rect_h;
    }
    GtImage gt_img[2];
    if (with_gt) {
        std::string why;
        if (!load_gt(gt_path[0], gt_scale, w, h, gt_img[0], why) || (!gt_path[1].empty() && !load_gt(gt_path[1], gt_scale, w, h, gt_img[1], why))) {
            printf("--gt refused: %s\n", why.c_str());
            return -1;
        }
    }
    std::vector<uint8> reg_bgr; // (the colour image of --register: B, G, R of the target camera)
    if (with_register && !reg_color.empty()) {
        int cw = 0, chh = 0;
        if (!load_image(reg_color.c_str(), reg_bgr, cw, chh) || cw != reg_target.width || chh != reg_target.height) {
            printf("--register refused: %s is not a readable image of the target's size\n", reg_color.c_str());
            return -1;
        }
    }
    printf("Done!\n");
    ADCensusOption ad_option;                               // main.cpp:80-92
    ad_option.min_disparity = argc < 4 ? 0 : atoi(argv[3]);
    ad_option.max_disparity = argc < 5 ? 64 : atoi(argv[4]);
    ad_option.lrcheck_thres = 1.0f;
    ad_option.do_lr_check = true;
    ad_option.do_filling = true;
    std::string out = argc < 6 ? std::string(argv[1]) : std::string(argv[5]);
    if (argc < 6 && out.size() > 4 && out[out.size() - 4] == '.') out.resize(out.size() - 4);
    printf("w = %d, h = %d, d = [%d,%d]\n\n", w, h, ad_option.min_disparity, ad_option.max_disparity);

    ADCensusStereo ad_census;
    ad_census.SetVerbose(true);
    printf("AD-Census Initializing...\n");
    auto t0 = std::chrono::steady_clock::now();
    if (!ad_census.Initialize(w, h, ad_option)) { printf("AD-Census initialisation failed: %s\n", ad_census.LastError()); return -2; }
    auto t1 = std::chrono::steady_clock::now();
    printf("AD-Census Initializing Done! Timing :	%lf s\n\n", std::chrono::duration<double>(t1 - t0).count());
    if (speckle_size > 0 && !ad_census.SetSpeckleFilter(speckle_size, speckle_diff)) { printf("speckle filter refused: %s\n", ad_census.LastError()); return -2; }
    if (with_voxel && !ad_census.SetCloudVoxelGrid(&voxel_grid)) { printf("voxel grid refused: %s\n", ad_census.LastError()); return -2; }
    std::vector<uint8> rect_left; // (the rectified left image: the colours of the cloud file)
    if (with_rectify || with_raw) {
        std::vector<uint8> rect_right((size_t)w * h * 3, 0), rgb((size_t)w * h * 3);
        rect_left.assign((size_t)w * h * 3, 0);
        const bool set = with_rectify ? ad_census.SetRectifyModel(ADC_SIDE_LEFT, &rect_file[0].raw, &rect_file[0].model) && ad_census.SetRectifyModel(ADC_SIDE_RIGHT, &rect_file[1].raw, &rect_file[1].model)
                                      : ad_census.SetInputFormat(ADC_SIDE_LEFT, &raw_fmt) && ad_census.SetInputFormat(ADC_SIDE_RIGHT, &raw_fmt);
        if (!set ||
            !ad_census.Rectify(ADC_SIDE_LEFT, left.data(), rect_left.data()) || !ad_census.Rectify(ADC_SIDE_RIGHT, right.data(), rect_right.data())) {
            printf("rectification refused: %s\n", ad_census.LastError());
            return -2;
        }
        for (int side = 0; side < 2; side++) {
            const std::vector<uint8>& img = side ? rect_right : rect_left;
            for (size_t i = 0; i < (size_t)w * h; i++) { rgb[3 * i] = img[3 * i + 2]; rgb[3 * i + 1] = img[3 * i + 1]; rgb[3 * i + 2] = img[3 * i]; }
            if (!write_png(out + (side ? "-rect-right.png" : "-rect-left.png"), rgb.data(), w, h, 3)) printf("cannot write %s-rect-*.png\n", out.c_str());
        }
    }
    printf("AD-Census Matching...\n");
    std::vector<float32> disparity((size_t)w * h, 0.0f);
    const bool with_maps = extras || with_tsdf_fuse; // (--tsdf-fuse weighs the map by the provenance and confidence of the same Match)
    std::vector<uint8> provenance(with_maps ? (size_t)w * h : 0);
    std::vector<float32> confidence(with_maps ? (size_t)w * h : 0);
    std::vector<float32> depth(with_calib ? (size_t)w * h : 0);
    std::vector<adc_point> cloud(with_calib ? (size_t)w * h : 0);
    adc_outputs outputs = {&calib, depth.data(), cloud.data(), cloud.size(), nullptr, nullptr};
    // --disp16: ONE Match through MatchProducts delivers the 16-bit map together with whatever the other options ask for
    std::vector<uint16_t> disp16(with_disp16 ? (size_t)w * h : 0);
    adc_products products = {with_maps ? provenance.data() : nullptr, with_maps ? confidence.data() : nullptr, {nullptr, nullptr, nullptr, 0, nullptr, nullptr},
                             with_disp16 ? disp16.data() : nullptr, disp16_scale, 0};
    if (with_calib) products.out = outputs;
    t0 = std::chrono::steady_clock::now();
    const bool ok = (with_disp16 || with_tsdf_fuse) ? ad_census.MatchProducts(left.data(), right.data(), disparity.data(), &products) : with_calib ? ad_census.MatchOut(left.data(), right.data(), disparity.data(), &outputs) : extras ? ad_census.MatchEx(left.data(), right.data(), disparity.data(), provenance.data(), confidence.data())
                           : ad_census.Match(left.data(), right.data(), disparity.data());
    if (!ok) { printf("AD-Census matching failed: %s\n", ad_census.LastError()); return -2; }
    t1 = std::chrono::steady_clock::now();
    printf("\nAD-Census Matching...Done! Timing :	%lf s\n", std::chrono::duration<double>(t1 - t0).count());

    // SaveDisparityMap (main.cpp:180-206): min-max over the valid |d|, uchar((|d| - min) / (max - min) * 255), invalid -> 0
    float32 mn = float32(w), mx = -float32(w);
    for (float32 d : disparity) { const float32 a = fabsf(d); if (a != Invalid_Float) { mn = a < mn ? a : mn; mx = a > mx ? a : mx; } }
    std::vector<uint8> gray((size_t)w * h, 0), col((size_t)w * h * 3, 0);
    for (size_t i = 0; i < gray.size(); i++) {
        const float32 a = fabsf(disparity[i]);
        // (a constant map has max == min: the reference divides 0 by 0 there, main.cpp:196 -- written as 0 instead of casting a NaN)
        gray[i] = (a == Invalid_Float || !(mx > mn)) ? 0 : static_cast<uint8>((a - mn) / (mx - mn) * 255);
        col[3 * i] = kJet[gray[i]][0]; col[3 * i + 1] = kJet[gray[i]][1]; col[3 * i + 2] = kJet[gray[i]][2];
    }
    if (!write_png(out + "-d.png", gray.data(), w, h, 1) || !write_png(out + "-c.png", col.data(), w, h, 3)) printf("cannot write %s-d.png / -c.png\n", out.c_str());
    // SaveDisparityCloud (main.cpp:212-230): x y |d| r g b, colours of the left image (stored B,G,R)
    FILE* f = fopen((out + "-cloud.txt").c_str(), "w");
    if (f && with_voxel) { // the voxel rows: x y z r g b of every voxel, in the order of the cloud
        adc_voxel_report vrep = {0, 0, 0};
        ad_census.GetVoxelReport(&vrep);
        printf("\nVoxel grid, leaf %g: %u valid points, %u kept, %u voxels\n", voxel_grid.leaf, vrep.points_valid, vrep.points_kept, vrep.voxels);
        const size_t count = (size_t)ad_census.CloudCount();
        for (size_t i = 0; i < count && i < cloud.size(); i++) fprintf(f, "%f %f %f %d %d %d\n", cloud[i].x, cloud[i].y, cloud[i].z, cloud[i].r, cloud[i].g, cloud[i].b);
        fclose(f);
    } else if (f) {
        for (int i = 0; i < h; i++)
            for (int j = 0; j < w; j++) {
                const float32 a = fabsf(disparity[(size_t)i * w + j]);
                if (a == Invalid_Float) continue;
                const uint8* p = (with_rectify || with_raw) ? &rect_left[((size_t)i * w + j) * 3] : &left[((size_t)i * w + j) * 3];
                fprintf(f, "%f %f %f %d %d %d\n", float32(j), float32(i), a, p[2], p[1], p[0]);
            }
        fclose(f);
    }
    write_pfm(out + ".pfm", disparity.data(), w, h);
    if (extras) {
        std::vector<uint8> conf8((size_t)w * h);
        for (size_t i = 0; i < conf8.size(); i++) conf8[i] = static_cast<uint8>(confidence[i] * 255);
        if (!write_png(out + "-prov.png", provenance.data(), w, h, 1) || !write_png(out + "-conf.png", conf8.data(), w, h, 1))
            printf("cannot write %s-prov.png / -conf.png\n", out.c_str());
        write_pfm(out + "-conf.pfm", confidence.data(), w, h);
    }
    if (with_gt) {
        std::vector<float32> err((size_t)w * h);
        std::vector<uint8> cls((size_t)w * h), rgb((size_t)w * h * 3);
        adc_eval_report rep;
        if (!ad_census.SetGroundTruth(&gt_img[0].gt, gt_path[1].empty() ? nullptr : &gt_img[1].gt, nullptr, 1.0f) ||
            !ad_census.Evaluate(disparity.data(), extras ? provenance.data() : nullptr, extras ? confidence.data() : nullptr, &eval_params, err.data(), cls.data(), &rep)) {
            printf("evaluation refused: %s\n", ad_census.LastError());
            return -2;
        }
        const int n = rep.n_thresholds;
        printf("\nEvaluation against %s (scale %g)%s\n%-14s %9s %8s", gt_path[0].c_str(), gt_scale, rep.has_right_gt ? ", non-occluded by cross-check within 1 px" : "",
               "mask", "pixels", "invalid%");
        for (int k = 0; k < n; k++) printf(" bad>%-4g%%", rep.thresholds[k]);
        printf(" %8s %8s\n", "mean", "rms");
        print_eval_row("all", rep.all.pixels, rep.all.invalid, rep.all.bad, n, rep.all.sum_err_q, &rep.all.sum_sq_err_q);
        if (rep.has_right_gt) print_eval_row("nonocc", rep.nonocc.pixels, rep.nonocc.invalid, rep.nonocc.bad, n, rep.nonocc.sum_err_q, &rep.nonocc.sum_sq_err_q);
        if (rep.has_provenance) {
            static const char* const names[4] = {"fill:wta", "fill:voting", "fill:interp", "fill:none"};
            for (int f = 0; f < 4; f++) print_eval_row(names[f], rep.by_fill[f].pixels, rep.by_fill[f].invalid, rep.by_fill[f].bad, n, rep.by_fill[f].sum_err_q, nullptr);
            if (speckle_size > 0) printf("known pixels removed by the speckle filter: %llu\n", (unsigned long long)rep.speckle_removed_known);
        }
        if (rep.has_confidence && n > 0) { // sparsification: bins from low confidence up, error rate of the pixels that remain
            double total = 0, total_bad = 0, removed = 0, removed_bad = 0, area = 0, x0 = 0, y0 = 0;
            for (int b = 0; b < ADC_EVAL_CONF_BINS; b++) { total += (double)rep.conf_pixels[b]; total_bad += (double)rep.conf_bad[b]; }
            y0 = total > 0 ? total_bad / total : 0;
            for (int b = 0; b < ADC_EVAL_CONF_BINS && total > 0; b++) {
                removed += (double)rep.conf_pixels[b];
                removed_bad += (double)rep.conf_bad[b];
                const double x1 = removed / total, y1 = total - removed > 0 ? (total_bad - removed_bad) / (total - removed) : 0;
                area += (x1 - x0) * (y0 + y1) / 2;
                x0 = x1; y0 = y1;
            }
            printf("confidence: sparsification area %.4f (random ranking %.4f) over %.0f measured pixels, bad > %g\n", area, total > 0 ? total_bad / total : 0, total,
                   rep.thresholds[0]);
        }
        for (size_t i = 0; i < cls.size(); i++) {
            const uint8 c = cls[i];
            const bool occ = (c & ADC_EVAL_OCCLUDED) != 0;
            uint8 r = 0, g = 0, b = 0;
            if (!(c & ADC_EVAL_KNOWN)) { }
            else if (!(c & ADC_EVAL_VALID)) { b = 255; }
            else if (c & ADC_EVAL_BAD) { r = 255; g = occ ? 160 : 0; }
            else { r = g = b = occ ? 140 : 220; }
            rgb[3 * i] = r; rgb[3 * i + 1] = g; rgb[3 * i + 2] = b;
        }
        write_pfm(out + "-err.pfm", err.data(), w, h);
        if (!write_png(out + "-bad.png", rgb.data(), w, h, 3)) printf("cannot write %s-bad.png\n", out.c_str());
    }
    if (with_disp16) { // binary PGM, maxval 65535: two bytes per sample, most significant first
        FILE* pgm = fopen((out + "-disp16.pgm").c_str(), "wb");
        if (pgm) {
            fprintf(pgm, "P5\n%d %d\n65535\n", w, h);
            std::vector<uint8> row((size_t)w * 2);
            for (int y = 0; y < h; y++) {
                for (int x = 0; x < w; x++) { const uint16_t v = disp16[(size_t)y * w + x]; row[2 * x] = (uint8)(v >> 8); row[2 * x + 1] = (uint8)(v & 0xff); }
                fwrite(row.data(), 1, row.size(), pgm);
            }
            fclose(pgm);
        } else printf("cannot write %s-disp16.pgm\n", out.c_str());
    }
    if (with_register) { // depth into the target camera; with a colour image the image aligned to the left view, which then colours the cloud
        const size_t pt = (size_t)reg_target.width * reg_target.height;
        std::vector<float32> reg_depth(pt);
        adc_reg_report rep;
        if (!ad_census.SetRegisterTarget(&reg_target) ||
            !ad_census.RegisterDepth(disparity.data(), ADC_REG_FROM_DISPARITY, &calib, 0, reg_depth.data(), nullptr, &rep)) {
            printf("registration refused: %s\n", ad_census.LastError());
            return -2;
        }
        printf("\nRegistered into %d x %d: %u valid source pixels, %u projected, %u target pixels filled\n", reg_target.width, reg_target.height, rep.src_valid,
               rep.src_projected, rep.dst_filled);
        write_pfm(out + "-reg.pfm", reg_depth.data(), reg_target.width, reg_target.height);
        if (!reg_bgr.empty()) {
            std::vector<uint8> aligned((size_t)w * h * 3), rgb((size_t)w * h * 3);
            if (!ad_census.AlignColor(disparity.data(), ADC_REG_FROM_DISPARITY, &calib, reg_bgr.data(), aligned.data(), nullptr)) {
                printf("registration refused: %s\n", ad_census.LastError());
                return -2;
            }
            for (size_t i = 0; i < (size_t)w * h; i++) { rgb[3 * i] = aligned[3 * i + 2]; rgb[3 * i + 1] = aligned[3 * i + 1]; rgb[3 * i + 2] = aligned[3 * i]; }
            if (!write_png(out + "-aligned.png", rgb.data(), w, h, 3)) printf("cannot write %s-aligned.png\n", out.c_str());
            // the cloud holds the valid pixels (a = |d| finite, a + doffs > 0) in raster order: the k-th of them is the k-th point
            // (a voxel cloud keeps the mean colours of the left image: a voxel is not a pixel)
            size_t k = 0;
            for (size_t i = 0; i < (size_t)w * h && k < cloud.size() && !with_voxel; i++) {
                const float32 a = fabsf(disparity[i]);
                if (!(std::isfinite(a) && a + calib.doffs > 0.0f)) continue;
                cloud[k].r = aligned[3 * i + 2]; cloud[k].g = aligned[3 * i + 1]; cloud[k].b = aligned[3 * i];
                k++;
            }
        }
    }
    std::vector<float32> point_normals; // (--normals without --voxel: three floats per cloud point)
    std::vector<float32> nrm;           // (--normals: four floats per pixel; the mesh gathers its vertex normals from it)
    if (with_normals) { // the normal map of the delivered disparity map; the host pairs normals and cloud points, which share the pixel
        nrm.resize((size_t)w * h * 4);
        std::vector<uint8> nrm8((size_t)w * h * 4), rgb((size_t)w * h * 3);
        adc_normals_report rep;
        if (!ad_census.Normals(disparity.data(), &calib, &normals_params, nrm.data(), nrm8.data(), &rep)) {
            printf("normals refused: %s\n", ad_census.LastError());
            return -2;
        }
        printf("\nNormals, radius %d: %u usable pixels, %u fitted, %u with too few points, %u degenerate\n", normals_params.radius, rep.usable, rep.fitted,
               rep.few_points, rep.degenerate);
        for (size_t i = 0; i < (size_t)w * h; i++) { rgb[3 * i] = nrm8[4 * i]; rgb[3 * i + 1] = nrm8[4 * i + 1]; rgb[3 * i + 2] = nrm8[4 * i + 2]; }
        if (!write_png(out + "-n.png", rgb.data(), w, h, 3)) printf("cannot write %s-n.png\n", out.c_str());
        if (!with_voxel) {
            // the cloud holds the valid pixels (a = |d| finite, a + doffs > 0) in raster order: the k-th of them is the k-th point
            for (size_t i = 0; i < (size_t)w * h; i++) {
                const float32 a = fabsf(disparity[i]);
                if (!(std::isfinite(a) && a + calib.doffs > 0.0f)) continue;
                point_normals.insert(point_normals.end(), nrm.begin() + 4 * i, nrm.begin() + 4 * i + 3);
            }
        }
    }
    if (with_mesh) { // the mesh of the delivered disparity map, sized at the lattice's worst case
        const size_t wl = (size_t)((w - 1) / mesh_params.step + 1), hl = (size_t)((h - 1) / mesh_params.step + 1);
        const size_t vcap = wl * hl, tcap = 2 * (wl - 1) * (hl - 1);
        std::vector<adc_point> vertices(vcap);
        std::vector<sint32> vertex_index(vcap);
        std::vector<uint32> triangles(3 * tcap + 3);
        adc_mesh_report rep;
        const uint8* colours = (with_rectify || with_raw) ? rect_left.data() : left.data();
        if (!ad_census.Mesh(disparity.data(), colours, with_calib ? &calib : nullptr, &mesh_params, vertices.data(), vcap, vertex_index.data(), triangles.data(), tcap,
                            &rep)) {
            printf("mesh refused: %s\n", ad_census.LastError());
            return -2;
        }
        printf("\nMesh, step %d: %u valid lattice pixels, %u vertices, %u triangles, %u cells of two, %u cells of one\n", mesh_params.step, rep.lattice_valid,
               rep.vertices, rep.triangles, rep.cells_two, rep.cells_one);
        FILE* ply = fopen((out + "-mesh.ply").c_str(), "wb");
        if (ply) {
            fprintf(ply, "ply\nformat binary_little_endian 1.0\nelement vertex %u\nproperty float x\nproperty float y\nproperty float z\n%s"
                         "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %u\nproperty list uchar int vertex_indices\nend_header\n",
                    rep.vertices, with_normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "", rep.triangles);
            for (size_t i = 0; i < rep.vertices; i++) {
                fwrite(&vertices[i].x, 4, 3, ply);
                if (with_normals) fwrite(&nrm[4 * (size_t)vertex_index[i]], 4, 3, ply);
                fwrite(&vertices[i].r, 1, 3, ply);
            }
            const uint8 three = 3;
            for (size_t i = 0; i < rep.triangles; i++) { fwrite(&three, 1, 1, ply); fwrite(&triangles[3 * i], 4, 3, ply); }
            fclose(ply);
        } else printf("cannot write %s-mesh.ply\n", out.c_str());
    }
    if (with_tsdf) { // the delivered disparity map and the left image fused into a fresh volume, then its surface points
        tsdf_frame.kind = ADC_REG_FROM_DISPARITY;
        tsdf_frame.calib = calib;
        adc_tsdf_report irep;
        adc_tsdf_extract_report xrep;
        const uint8* colours = (with_rectify || with_raw) ? rect_left.data() : left.data();
        std::vector<adc_point> points;
        adc_tsdf_weight_report wrep;
        adc_tsdf_fuse_report frep;
        std::vector<uint8> weight(with_tsdf_fuse ? (size_t)w * h : 0);
        bool ok = ad_census.TsdfCreate(&tsdf_params);
        if (ok && with_tsdf_fuse) { // the weights of this Match's own provenance and confidence, then the weighted frame
            ok = ad_census.TsdfWeights(disparity.data(), provenance.data(), confidence.data(), &tsdf_frame, &fuse_weights, weight.data(), &wrep) &&
                 ad_census.TsdfFuse(disparity.data(), colours, weight.data(), &tsdf_frame, &fuse_params, &frep);
            memset(&irep, 0, sizeof(irep));
            irep.in_frustum = frep.in_frustum; irep.no_depth = frep.no_depth; irep.occluded = frep.occluded; irep.updated = frep.updated;
        } else if (ok) ok = ad_census.TsdfIntegrate(disparity.data(), colours, &tsdf_frame, &irep);
        std::vector<adc_point> left_points;
        adc_tsdf_shift_report srep;
        memset(&srep, 0, sizeof(srep));
        if (ok && with_tsdf_shift) { // the window moves; what leaves it is a sub-list of the whole volume's points, which sizes the buffer
            adc_tsdf_extract_params all = tsdf_extract;
            all.min_weight = tsdf_shift.min_weight;
            ok = ad_census.TsdfExtract(&all, nullptr, 0, &xrep);
            left_points.resize(ok ? xrep.points : 0);
            ok = ok && ad_census.TsdfShift(&tsdf_shift, left_points.empty() ? nullptr : left_points.data(), left_points.size(), &srep) && srep.points <= left_points.size();
            sint32 offset[3] = {0, 0, 0};
            float32 origin0[3] = {0.0f, 0.0f, 0.0f};
            ok = ok && ad_census.TsdfGetOffset(offset, origin0);
            if (ok) {
                left_points.resize(srep.points);
                for (int a = 0; a < 3; a++) { // (the volume's origin now, by its definition: what the ray cast's and the track's defaults read)
                    const float32 step = (float32)offset[a] * tsdf_params.voxel;
                    tsdf_params.origin[a] = origin0[a] + step;
                }
            }
        }
        ok = ok && ad_census.TsdfExtract(&tsdf_extract, nullptr, 0, &xrep); // (counts only: the file is sized by the report)
        if (ok && xrep.points) {
            points.resize(xrep.points);
            ok = ad_census.TsdfExtract(&tsdf_extract, points.data(), points.size(), &xrep) && xrep.points == points.size();
        }
        if (!ok) {
            printf("tsdf refused: %s\n", ad_census.LastError());
            return -2;
        }
        printf("\nTSDF: %u voxels in the frustum, %u without depth, %u occluded, %u updated; %u voxels seen, %u surface points\n", irep.in_frustum, irep.no_depth,
               irep.occluded, irep.updated, xrep.voxels_seen, xrep.points);
        if (with_tsdf_fuse)
            printf("TSDF fuse: %u pixels with depth, %u weighted, %u below the confidence, %u saturated; %u voxels unweighted, %u interpolated\n", wrep.valid, wrep.nonzero,
                   wrep.below_confidence, wrep.saturated, frep.unweighted, frep.interpolated);
        if (with_tsdf_shift) {
            printf("TSDF shift %d,%d,%d: %u voxels moved, %u left, %u of them seen; %u leaving surface points\n", tsdf_shift.shift[0], tsdf_shift.shift[1], tsdf_shift.shift[2],
                   srep.moved_nonempty, srep.left_nonempty, srep.left_seen, srep.points);
            FILE* lply = fopen((out + "-tsdf-left.ply").c_str(), "wb");
            if (lply) {
                fprintf(lply, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
                              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n", left_points.size());
                for (size_t i = 0; i < left_points.size(); i++) {
                    fwrite(&left_points[i].x, 4, 3, lply);
                    fwrite(&left_points[i].r, 1, 3, lply);
                }
                fclose(lply);
            } else printf("cannot write %s-tsdf-left.ply\n", out.c_str());
        }
        FILE* ply = fopen((out + "-tsdf.ply").c_str(), "wb");
        if (ply) {
            fprintf(ply, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
                         "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n", points.size());
            for (size_t i = 0; i < points.size(); i++) {
                fwrite(&points[i].x, 4, 3, ply);
                fwrite(&points[i].r, 1, 3, ply);
            }
            fclose(ply);
        } else printf("cannot write %s-tsdf.ply\n", out.c_str());
        if (with_tsdf_mesh) { // the same volume as a triangle mesh: the vertex list is the point list above
            adc_tsdf_mesh_report mrep;
            std::vector<adc_point> vertices;
            std::vector<uint32> triangles;
            adc_point no_vertex;
            uint32 no_triangle = 0;
            ok = ad_census.TsdfMesh(&tsdf_extract, &no_vertex, 0, &no_triangle, 0, &mrep); // (counts only: the file is sized by the report)
            if (ok && (mrep.vertices || mrep.triangles)) {
                vertices.resize(mrep.vertices ? mrep.vertices : 1);
                triangles.resize(mrep.triangles ? 3 * (size_t)mrep.triangles : 3);
                const uint32 nv = mrep.vertices, nt = mrep.triangles;
                ok = ad_census.TsdfMesh(&tsdf_extract, vertices.data(), nv, triangles.data(), nt, &mrep) && mrep.vertices == nv && mrep.triangles == nt;
            }
            if (!ok) {
                printf("tsdf mesh refused: %s\n", ad_census.LastError());
                return -2;
            }
            printf("TSDF mesh: %u voxels seen, %u vertices, %u triangles, %u cells seen, %u surface cells\n", mrep.voxels_seen, mrep.vertices, mrep.triangles,
                   mrep.cells_seen, mrep.cells_surface);
            ply = fopen((out + "-tsdf-mesh.ply").c_str(), "wb");
            if (ply) {
                fprintf(ply, "ply\nformat binary_little_endian 1.0\nelement vertex %u\nproperty float x\nproperty float y\nproperty float z\n"
                             "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %u\nproperty list uchar int vertex_indices\nend_header\n",
                        mrep.vertices, mrep.triangles);
                for (size_t i = 0; i < mrep.vertices; i++) {
                    fwrite(&vertices[i].x, 4, 3, ply);
                    fwrite(&vertices[i].r, 1, 3, ply);
                }
                const uint8 three = 3;
                for (size_t i = 0; i < mrep.triangles; i++) { fwrite(&three, 1, 1, ply); fwrite(&triangles[3 * i], 4, 3, ply); }
                fclose(ply);
            } else printf("cannot write %s-tsdf-mesh.ply\n", out.c_str());
        }
        if (with_tsdf_raycast) { // the same volume seen from the view's pose: depth and normals, the normal image made here
            if (!with_view_pose) {
                memcpy(ray_view.R, tsdf_frame.R, sizeof(ray_view.R));
                memcpy(ray_view.t, tsdf_frame.t, sizeof(ray_view.t));
            }
            if (!(ray_view.step > 0.0f)) ray_view.step = tsdf_params.voxel * 0.5f;
            if (!(ray_view.skip > 0.0f)) ray_view.skip = tsdf_params.trunc * 0.5f > ray_view.step ? tsdf_params.trunc * 0.5f : ray_view.step;
            ray_view.z_near = tsdf_params.voxel;
            ray_view.z_far = 3.0e38f; // (the volume's box ends every ray)
            ray_view.min_weight = tsdf_extract.min_weight;
            ray_view.max_steps = 16384;
            const size_t rp = (size_t)ray_view.width * ray_view.height;
            std::vector<float32> ray_depth(rp), ray_normals(4 * rp);
            std::vector<uint8> ray_rgb(3 * rp);
            adc_tsdf_raycast_report rrep;
            if (!ad_census.TsdfRaycast(&ray_view, ray_depth.data(), ray_normals.data(), nullptr, nullptr, &rrep)) {
                printf("tsdf raycast refused: %s\n", ad_census.LastError());
                return -2;
            }
            printf("TSDF raycast: %u rays, %u miss, %u hit, %u no surface, %u behind, %u exhausted, %llu samples\n", rrep.rays, rrep.miss, rrep.hit, rrep.no_surface,
                   rrep.behind, rrep.exhausted, (unsigned long long)rrep.samples_lo | ((unsigned long long)rrep.samples_hi << 32));
            for (size_t i = 0; i < rp; i++)
                for (int k = 0; k < 3; k++)
                    ray_rgb[3 * i + k] = ray_normals[4 * i + 3] > 0.0f ? (uint8)((int)rintf(ray_normals[4 * i + k] * 127.0f) + 128) : 0;
            write_pfm(out + "-ray.pfm", ray_depth.data(), ray_view.width, ray_view.height);
            if (!write_png(out + "-ray-n.png", ray_rgb.data(), ray_view.width, ray_view.height, 3)) printf("cannot write %s-ray-n.png\n", out.c_str());
        }
        if (with_tsdf_track) { // a second frame tracked against the volume that now holds the pair's map
            std::vector<float32> second;
            int tw = 0, th = 0;
            if (!load_pfm(track_map, second, tw, th) || tw != w || th != h) {
                printf("tsdf track refused: cannot read %s as a one-channel PFM of %d x %d pixels\n", track_map.c_str(), w, h);
                return -2;
            }
            adc_tsdf_frame guess = tsdf_frame;
            if (with_track_guess) {
                for (int k = 0; k < 9; k++) guess.R[k] = track_guess[k];
                for (int k = 0; k < 3; k++) guess.t[k] = track_guess[9 + k];
            }
            // the API's defaults, but z_far: nothing in the volume is farther from the guess camera than the volume's farthest corner
            adc_track_params tp = {10u, 1u, 0.1f, 0.8f, 8.0f, 64u, 1.0e-5f, 1.0e-5f, 0.5f, 0.5f, 0.0f, 1.0e-6f, 0u, {0u, 0u, 0u}};
            double centre[3], far2 = 0.0;
            for (int a = 0; a < 3; a++)
                centre[a] = -((((double)guess.R[a] * (double)guess.t[0]) + ((double)guess.R[3 + a] * (double)guess.t[1])) + ((double)guess.R[6 + a] * (double)guess.t[2]));
            const int dims[3] = {tsdf_params.nx, tsdf_params.ny, tsdf_params.nz};
            for (int corner = 0; corner < 8; corner++) {
                double d2 = 0.0;
                for (int a = 0; a < 3; a++) {
                    const double d = ((double)tsdf_params.origin[a] + ((double)(((corner >> a) & 1) ? dims[a] : 0) * (double)tsdf_params.voxel)) - centre[a];
                    d2 = d2 + (d * d);
                }
                if (d2 > far2) far2 = d2;
            }
            tp.z_far = (float)sqrt(far2);
            adc_track_result tr;
            if (!ad_census.TsdfTrack(second.data(), &guess, &tp, &tr) || tr.solves < 1 || tr.solves > ADC_TRACK_MAX_ITERATIONS_LIMIT || tr.status > ADC_TRACK_DIVERGED) {
                printf("tsdf track refused: %s\n", ad_census.LastError());
                return -2;
            }
            static const char* const status_name[5] = {"converged", "max iterations", "lost", "degenerate", "diverged"};
            const adc_track_iteration& last = tr.iteration[tr.solves - 1];
            printf("TSDF track: %s after %u solves, %u of %u pixels used, rms %.9g, last step %.9g rad %.9g\n", status_name[tr.status], tr.solves, tr.used, tr.pixels,
                   last.rms, last.rot, last.trans);
            FILE* tf = fopen((out + "-track.txt").c_str(), "w");
            if (tf) {
                for (int k = 0; k < 9; k++) fprintf(tf, "%.9g\n", tr.R[k]);
                for (int k = 0; k < 3; k++) fprintf(tf, "%.9g\n", tr.t[k]);
                fclose(tf);
            } else printf("cannot write %s-track.txt\n", out.c_str());
        }
    }
    if (with_calib) {
        write_pfm(out + "-depth.pfm", depth.data(), w, h);
        const size_t count = (size_t)ad_census.CloudCount();
        const bool ply_normals = with_normals && !with_voxel && point_normals.size() >= 3 * count;
        FILE* ply = fopen((out + "-cloud.ply").c_str(), "wb");
        if (ply) {
            fprintf(ply, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n%s"
                         "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n", count,
                    ply_normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "");
            for (size_t i = 0; i < count; i++) {
                fwrite(&cloud[i].x, 4, 3, ply);
                if (ply_normals) fwrite(&point_normals[3 * i], 4, 3, ply);
                fwrite(&cloud[i].r, 1, 3, ply);
            }
            fclose(ply);
        } else printf("cannot write %s-cloud.ply\n", out.c_str());
    }
    return 0;
}
