// yk_mitsuba.cpp — the reference's Mitsuba 2.1.0 scene loader and the by-extension dispatch of its front end.
//
//   scene::mitsuba::load            yuki/src/scene/mitsuba/mod.rs:28-218
//   parse_element!, find_attr!      scene/mitsuba/macros.rs
//   sensor / shape / material / emitter / transform / common::parse_rgb   scene/mitsuba/*.rs
//   try_load_scene                  yuki/src/app/util.rs:15-63
//
// Behaviour follows the reference statement by statement, quirks included: every mesh, spot light and the camera go through
// scale(-1, 1, 1) ("Mitsuba's +X is to the left of +Z"), a `twosided` parses any nested bsdf as `diffuse`, `<point>` expects
// `name` as its first attribute, lists are split on single spaces, the camera target moves to the middle of the scene's
// bounds.  Where the reference panics (unwrap, index, unreachable!, assert) the call returns an error.  The reference reads
// XML through the xml-rs crate, which is not part of its tree; XmlReader below restates XML 1.0 as far as such files use
// it.  On a well-formedness error the reference logs and STOPS READING (mod.rs:179-182, macros.rs:100-103): every nesting
// level leaves its loop and finishes with what it has.  That is kept.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "../../include/yuki_hip.h"
#include "yk_bsdf.h"
#include "yk_host.h"
#include "yk_libm.h"
#include "yk_loaders_internal.h"
#include "yk_math.h"

using namespace yk;

namespace {

struct Fail {
    yk_status st;
    std::string msg;
};
[[noreturn]] void fail(const std::string& msg, yk_status st = YK_ERR_INVALID_ARGUMENT) { throw Fail{st, msg}; }

// ------------------------------------------------------------------ XML events
struct Attr {
    std::string name, value;
};
struct Ev {
    enum Kind { Start, End, Chars, Space, CData, PI, Doctype, EndDoc, Error } kind = Error;
    std::string name;  // element / PI target; text for Chars and CData
    std::vector<Attr> attrs;
};

bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
bool name_start(unsigned char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_' || c == ':' || c >= 0x80; }
bool name_char(unsigned char c) { return name_start(c) || (c >= '0' && c <= '9') || c == '-' || c == '.'; }

// A pull reader over the whole file.  An error is sticky: every later call returns Error again, as xml-rs does.
struct XmlReader {
    std::string in;
    size_t pos = 0;
    std::vector<std::string> open;
    bool failed = false, seen_root = false, pending_end = false;

    Ev error() {
        failed = true;
        return Ev();
    }
    bool starts(const char* s) const { return in.compare(pos, std::strlen(s), s) == 0; }
    // the five predefined entities and numeric character references; false on anything else
    bool decode(const std::string& raw, bool attribute, std::string& out) const {
        out.clear();
        for (size_t i = 0; i < raw.size(); ++i) {
            char c = raw[i];
            if (c != '&') {
                out.push_back(attribute && (c == '\t' || c == '\n' || c == '\r') ? ' ' : c);  // attribute-value normalisation
                continue;
            }
            size_t e = raw.find(';', i);
            if (e == std::string::npos) return false;
            std::string ent = raw.substr(i + 1, e - i - 1);
            if (ent == "lt") out.push_back('<');
            else if (ent == "gt") out.push_back('>');
            else if (ent == "amp") out.push_back('&');
            else if (ent == "apos") out.push_back('\'');
            else if (ent == "quot") out.push_back('"');
            else if (ent.size() >= 2 && ent[0] == '#') {
                const bool hex = ent[1] == 'x';
                const std::string digits = ent.substr(hex ? 2 : 1);
                if (digits.empty() || digits.size() > 8) return false;
                for (char d : digits)
                    if (!((d >= '0' && d <= '9') || (hex && ((d >= 'a' && d <= 'f') || (d >= 'A' && d <= 'F'))))) return false;
                unsigned long cp = std::strtoul(digits.c_str(), nullptr, hex ? 16 : 10);
                if (cp == 0 || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF) || (cp < 0x20 && cp != 9 && cp != 10 && cp != 13)) return false;
                if (cp < 0x80) out.push_back((char)cp);
                else if (cp < 0x800) { out.push_back((char)(0xC0 | (cp >> 6))); out.push_back((char)(0x80 | (cp & 63))); }
                else if (cp < 0x10000) { out.push_back((char)(0xE0 | (cp >> 12))); out.push_back((char)(0x80 | ((cp >> 6) & 63))); out.push_back((char)(0x80 | (cp & 63))); }
                else { out.push_back((char)(0xF0 | (cp >> 18))); out.push_back((char)(0x80 | ((cp >> 12) & 63))); out.push_back((char)(0x80 | ((cp >> 6) & 63))); out.push_back((char)(0x80 | (cp & 63))); }
            } else return false;
            i = e;
        }
        return true;
    }
    bool read_name(std::string& out) {
        size_t st = pos;
        if (pos >= in.size() || !name_start((unsigned char)in[pos])) return false;
        while (pos < in.size() && name_char((unsigned char)in[pos])) ++pos;
        out = in.substr(st, pos - st);
        return true;
    }
    void skip_space() {
        while (pos < in.size() && is_space(in[pos])) ++pos;
    }

    Ev next() {
        if (failed) return Ev();
        Ev ev;
        if (pending_end) {  // the second half of an empty-element tag
            pending_end = false;
            ev.kind = Ev::End;
            ev.name = open.back();
            open.pop_back();
            return ev;
        }
        for (;;) {
            if (pos >= in.size()) {
                if (!open.empty() || !seen_root) return error();  // the file ends inside an element
                ev.kind = Ev::EndDoc;
                return ev;
            }
            if (in[pos] != '<') {  // character data up to the next markup
                size_t e = in.find('<', pos);
                if (e == std::string::npos) e = in.size();
                std::string raw = in.substr(pos, e - pos), text;
                pos = e;
                bool blank = true;
                for (char c : raw) blank = blank && is_space(c);
                if (open.empty()) {  // outside the root only white space may appear
                    if (!blank) return error();
                    continue;
                }
                if (blank) continue;  // XmlEvent::Whitespace: skipped by every loop of the reference
                if (raw.find("]]>") != std::string::npos || !decode(raw, false, text)) return error();
                ev.kind = Ev::Chars;
                ev.name = text;
                return ev;
            }
            if (starts("<!--")) {
                size_t e = in.find("--", pos + 4);
                if (e == std::string::npos || in.compare(e, 3, "-->") != 0) return error();  // "--" inside a comment is malformed
                pos = e + 3;
                continue;
            }
            if (starts("<![CDATA[")) {
                size_t e = in.find("]]>", pos + 9);
                if (open.empty() || e == std::string::npos) return error();
                ev.kind = Ev::CData;
                ev.name = in.substr(pos + 9, e - pos - 9);
                pos = e + 3;
                return ev;
            }
            if (starts("<?")) {
                size_t st = pos;
                pos += 2;
                std::string target;
                if (!read_name(target)) return error();
                size_t e = in.find("?>", pos);
                if (e == std::string::npos) return error();
                pos = e + 2;
                std::string low = target;
                for (char& c : low) c = (char)std::tolower((unsigned char)c);
                if (low == "xml") {  // the XML declaration: only at the very start of the file
                    if (st != 0 || target != "xml") return error();
                    continue;
                }
                ev.kind = Ev::PI;
                ev.name = target;
                return ev;
            }
            if (starts("<!DOCTYPE")) {
                ev.kind = Ev::Doctype;
                failed = true;
                return ev;
            }
            if (starts("</")) {
                pos += 2;
                std::string name;
                if (!read_name(name)) return error();
                skip_space();
                if (pos >= in.size() || in[pos] != '>') return error();
                ++pos;
                if (open.empty() || open.back() != name) return error();  // an end tag that does not match
                open.pop_back();
                ev.kind = Ev::End;
                ev.name = name;
                return ev;
            }
            // start tag or empty-element tag
            ++pos;
            if (!read_name(ev.name)) return error();
            if (open.empty() && seen_root) return error();  // a second root element
            for (;;) {
                const size_t before = pos;
                skip_space();
                if (pos >= in.size()) return error();
                if (in[pos] == '>') {
                    ++pos;
                    break;
                }
                if (in[pos] == '/') {
                    if (pos + 1 >= in.size() || in[pos + 1] != '>') return error();
                    pos += 2;
                    pending_end = true;
                    break;
                }
                if (pos == before) return error();  // attributes are separated by white space
                Attr a;
                if (!read_name(a.name)) return error();
                skip_space();
                if (pos >= in.size() || in[pos] != '=') return error();
                ++pos;
                skip_space();
                if (pos >= in.size() || (in[pos] != '"' && in[pos] != '\'')) return error();
                const char quote = in[pos++];
                size_t e = in.find(quote, pos);
                if (e == std::string::npos) return error();
                std::string raw = in.substr(pos, e - pos);
                pos = e + 1;
                if (raw.find('<') != std::string::npos || !decode(raw, true, a.value)) return error();
                for (const Attr& b : ev.attrs)
                    if (b.name == a.name) return error();  // a repeated attribute
                ev.attrs.push_back(a);
            }
            seen_root = true;
            open.push_back(ev.name);
            ev.kind = Ev::Start;
            return ev;
        }
    }
};

// ------------------------------------------------------------------ attributes and numbers
// try_find_attr! (macros.rs:2-12): the LAST attribute of that name
const std::string* try_find_attr(const std::vector<Attr>& attrs, const char* name) {
    const std::string* v = nullptr;
    for (const Attr& a : attrs)
        if (a.name == name) v = &a.value;
    return v;
}
// find_attr! (macros.rs:15-22)
const std::string& find_attr(const std::vector<Attr>& attrs, const char* name) {
    const std::string* v = try_find_attr(attrs, name);
    if (!v) fail(std::string("Could not find element attribute '") + name + "'");
    return *v;
}
// str::parse::<f32>(): Rust's grammar, then the correctly rounded value
float parse_f32(const std::string& v, const std::string& element) {
    if (!rust_float_grammar(v)) fail("invalid float literal '" + v + "' in element '" + element + "'");
    return std::strtof(v.c_str(), nullptr);
}
// str::parse::<u16>(): [+]digits, at most 65535
uint16_t parse_u16(const std::string& v, const std::string& element) {
    size_t i = (!v.empty() && v[0] == '+') ? 1 : 0;
    uint32_t n = 0;
    bool ok = i < v.size();
    for (; i < v.size() && ok; ++i) {
        ok = v[i] >= '0' && v[i] <= '9';
        if (ok) n = n * 10 + (uint32_t)(v[i] - '0');
        ok = ok && n <= 65535;
    }
    if (!ok) fail("invalid integer '" + v + "' in element '" + element + "'");
    return (uint16_t)n;
}
// value.split(' ').map(parse::<f32>): two spaces in a row give an empty piece, which does not parse
std::vector<float> parse_list(const std::string& v, const std::string& element) {
    std::vector<float> out;
    size_t st = 0;
    for (;;) {
        size_t e = v.find(' ', st);
        out.push_back(parse_f32(v.substr(st, e == std::string::npos ? std::string::npos : e - st), element));
        if (e == std::string::npos) return out;
        st = e + 1;
    }
}
// common::parse_rgb (common.rs:4-18): fewer than three components leave the rest zero, more than three index past the end
void parse_rgb(const std::vector<Attr>& attrs, const char* expected, float out[3]) {
    const std::string& name = find_attr(attrs, "name");
    if (name != expected) fail(std::string("Expected rgb to be '") + expected + "', got '" + name + "'");
    std::vector<float> c = parse_list(find_attr(attrs, "value"), std::string("rgb ") + expected);
    if (c.size() > 3) fail(std::string("rgb '") + expected + "' has more than three components");
    out[0] = out[1] = out[2] = 0.0f;
    for (size_t i = 0; i < c.size(); ++i) out[i] = c[i];
}

// ------------------------------------------------------------------ parse_element! (macros.rs:32-107)
// body(name, attributes, level, ignore_level) is called for every start tag that is not being ignored; it may set
// ignore_level = 0 to skip the element with its subtree, and lowers level after a nested parser consumed the element's end.
// Returns when the end tag of the element this parser was entered for is read, or when the reader fails.
template <class Body>
void parse_element(XmlReader& rd, Body body) {
    int level = 0;
    int64_t ignore_level = -1;  // Option<u32>: -1 = None
    for (;;) {
        Ev e = rd.next();
        switch (e.kind) {
            case Ev::Start:
                if (ignore_level < 0) body(e.name, e.attrs, level, ignore_level);
                level += 1;
                if (ignore_level >= 0) ignore_level += 1;
                break;
            case Ev::End:
                if (ignore_level >= 0) {
                    const int64_t level_after = ignore_level - 1;
                    ignore_level = level_after > 0 ? level_after : -1;
                }
                level -= 1;
                if (level < 0) return;
                break;
            case Ev::PI: fail("Unexpected processing instruction: " + e.name);
            case Ev::CData: fail("Unexpected CDATA: " + e.name);
            case Ev::Chars: fail("Unexpected characters outside tags: " + e.name);
            case Ev::Doctype: fail("DOCTYPE declarations are not supported", YK_ERR_UNSUPPORTED);
            case Ev::Space: break;
            case Ev::EndDoc:
            case Ev::Error: return;  // "XML error": stop reading, finish with what has been read
        }
    }
}

const float RADS_PER_DEG = YK_PI / 180.0f;  // f32::to_radians

// transform::parse (transform.rs:14-81): every child pre-multiplies
Xf parse_transform(XmlReader& rd) {
    Xf transform = xf_identity();
    parse_element(rd, [&](const std::string& name, const std::vector<Attr>& attrs, int&, int64_t&) {
        if (name == "rotate") {
            V3 axis{0.0f, 0.0f, 0.0f};
            if (auto v = try_find_attr(attrs, "x")) axis.x = parse_f32(*v, "rotate");
            if (auto v = try_find_attr(attrs, "y")) axis.y = parse_f32(*v, "rotate");
            if (auto v = try_find_attr(attrs, "z")) axis.z = parse_f32(*v, "rotate");
            axis = normalize(axis);
            const float angle = parse_f32(find_attr(attrs, "angle"), "rotate") * RADS_PER_DEG;
            transform = xf_mul(loader_rotation(angle, axis), transform);
        } else if (name == "translate") {
            std::vector<float> p = parse_list(find_attr(attrs, "value"), "translate");
            if (p.size() < 3) fail("translate needs three numbers");  // reference: index out of bounds
            transform = xf_mul(xf_translation(p[0], p[1], p[2]), transform);
        } else if (name == "scale") {
            // the pieces are counted before any of them is parsed (transform.rs:56-64)
            const std::string& v = find_attr(attrs, "value");
            size_t pieces = 1;
            for (char c : v) pieces += c == ' ';
            if (pieces != 1 && pieces != 3) fail("scale needs one or three numbers");  // reference: unreachable!()
            std::vector<float> p = parse_list(v, "scale");
            if (pieces == 1) p = {p[0], p[0], p[0]};
            transform = xf_mul(xf_scale(p[0], p[1], p[2]), transform);
        } else if (name == "matrix") {
            std::vector<float> m = parse_list(find_attr(attrs, "value"), "matrix");
            if (m.size() != 16) fail("matrix needs 16 numbers");  // reference: assert!(m.len() == 16)
            bool ok = true;
            Xf t = xf_from_matrix(m.data(), &ok);
            if (!ok) fail("matrix is singular");  // reference: "Can't invert, singular matrix"
            transform = xf_mul(t, transform);
        } else {
            fail("Unknown transformation data type '" + name + "'");
        }
    });
    return transform;
}

// approx::relative_eq! with its f32 defaults (epsilon = max_relative = f32::EPSILON)
bool relative_eq(float a, float b) {
    if (a == b) return true;
    if (std::isinf(a) || std::isinf(b)) return false;
    const float eps = 1.1920929e-7f;
    const float abs_diff = fabsf(a - b);
    if (abs_diff <= eps) return true;
    const float aa = fabsf(a), ab = fabsf(b);
    const float largest = ab > aa ? ab : aa;
    return abs_diff <= largest * eps;
}

Xf rotation_axis(int axis, float theta) {  // rotation_x / _y / _z, transforms.rs:46-94
    const float c = det_cosf(theta), s = det_sinf(theta);
    Xf t = xf_identity();
    if (axis == 0) { t.m[5] = c; t.m[6] = -s; t.m[9] = s; t.m[10] = c; }
    else if (axis == 1) { t.m[0] = c; t.m[2] = s; t.m[8] = -s; t.m[10] = c; }
    else { t.m[0] = c; t.m[1] = -s; t.m[4] = s; t.m[5] = c; }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) t.mi[4 * i + j] = t.m[4 * j + i];
    return t;
}

// sensor::parse (sensor.rs:18-109)
void parse_sensor(XmlReader& rd, yk_camera_params& cam) {
    std::string fov_axis;
    float fov_angle = 0.0f;
    Xf transform = xf_identity();
    parse_element(rd, [&](const std::string& name, const std::vector<Attr>& attrs, int& level, int64_t& ignore_level) {
        if (name == "string") {
            const std::string& n = find_attr(attrs, "name");
            const std::string& v = find_attr(attrs, "value");
            if (n == "fov_axis") fov_axis = v;
            else fail("Unknown sensor string element '" + n + "'");
        } else if (name == "float") {
            const std::string& n = find_attr(attrs, "name");
            const std::string& v = find_attr(attrs, "value");
            if (n == "fov") fov_angle = parse_f32(v, "float fov");
            else if (n == "near_clip" || n == "far_clip" || n == "") {
            } else fail("Unknown sensor string element '" + n + "'");
        } else if (name == "transform") {
            transform = parse_transform(rd);
            level -= 1;
        } else if (name == "sampler" || name == "film") {
            ignore_level = 0;
        } else {
            fail("Unknown sensor data type '" + name + "'");
        }
    });
    transform = xf_mul(xf_scale(-1.0f, 1.0f, 1.0f), transform);
    // Matrix4x4::decompose (math/matrix.rs:218-255)
    const float* m = transform.m;
    const float position[3] = {m[3], m[7], m[11]};
    const float sx = length(V3{m[0], m[4], m[8]}), sy = length(V3{m[1], m[5], m[9]}), sz = length(V3{m[2], m[6], m[10]});
    if (sx == 0.0f || sy == 0.0f || sz == 0.0f) fail("Cannot decompose camera to world matrix: Cannot decompose matrix with a zero scale component");
    const float mr[3][3] = {{m[0] / sx, m[1] / sy, m[2] / sz}, {m[4] / sx, m[5] / sy, m[6] / sz}, {m[8] / sx, m[9] / sy, m[10] / sz}};
    const float theta_x = det_atan2f(mr[1][2], mr[2][2]);
    const float c2 = sqrtf(mr[0][0] * mr[0][0] + mr[0][1] * mr[0][1]);
    const float theta_y = det_atan2f(-mr[0][2], c2);
    const float s1 = det_sinf(theta_x), c1 = det_cosf(theta_x);
    const float theta_z = det_atan2f(s1 * mr[2][0] - c1 * mr[1][0], c1 * mr[1][1] - s1 * mr[2][1]);
    if (!(relative_eq(sx, 1.0f) && relative_eq(sy, 1.0f) && relative_eq(sz, 1.0f))) fail("Camera to world has scaling");
    uint32_t axis = 0;
    if (fov_axis == "x") axis = 0;
    else if (fov_axis == "y") axis = 1;
    else fail("Unknown fov axis '" + fov_axis + "'");
    // "We compensate for the flipped X axis in the rotation"; rotation_euler = Rx * (Ry * Rz), transforms.rs:130-135
    Xf euler = xf_mul(rotation_axis(0, -theta_x), xf_mul(rotation_axis(1, -theta_y), rotation_axis(2, theta_z)));
    Xf c2w = xf_mul(xf_translation(position[0], position[1], position[2]), euler);
    V3 target = xf_point(c2w.m, V3{0.0f, 0.0f, 1.0f});
    V3 up = xf_vector(c2w.m, V3{0.0f, 1.0f, 0.0f});
    for (int k = 0; k < 3; ++k) cam.position[k] = position[k];
    cam.target[0] = target.x; cam.target[1] = target.y; cam.target[2] = target.z;
    cam.up[0] = up.x; cam.up[1] = up.y; cam.up[2] = up.z;
    cam.fov_axis = axis;
    cam.fov_degrees = fov_angle;
}

// material::parse_diffuse (material.rs:51-77)
yk_material_desc parse_diffuse(XmlReader& rd) {
    float reflectance[3] = {0.5f, 0.5f, 0.5f};
    parse_element(rd, [&](const std::string& name, const std::vector<Attr>& attrs, int&, int64_t&) {
        if (name == "rgb") parse_rgb(attrs, "reflectance", reflectance);
        else fail("Unknown light data type '" + name + "'");  // sic
    });
    return make_mat(YK_MAT_MATTE, reflectance, nullptr, 0.0f, false);
}
// material::parse_twosided (material.rs:17-49): a nested bsdf of ANY type is read as diffuse
yk_material_desc parse_twosided(XmlReader& rd) {
    const float ones[3] = {1.0f, 1.0f, 1.0f};
    yk_material_desc material = make_mat(YK_MAT_MATTE, ones, nullptr, 0.0f, false);
    parse_element(rd, [&](const std::string& name, const std::vector<Attr>& attrs, int& level, int64_t&) {
        if (name == "bsdf") {
            material = parse_diffuse(rd);
            level -= 1;
        } else if (name == "rgb") {
            float c[3];
            parse_rgb(attrs, "reflectance", c);
            material = make_mat(YK_MAT_MATTE, c, nullptr, 0.0f, false);
        } else {
            fail("Unknown material data type '" + name + "'");
        }
    });
    return material;
}
// material::parse_dielectric (material.rs:79-142)
const float BK7_GLASS_IOR = 1.5046f;
const float AIR_IOR = 1.000277f;
const float EXT_IOR_EPSILON = 0.001f;
yk_material_desc parse_dielectric(XmlReader& rd) {
    float int_ior = BK7_GLASS_IOR, ext_ior = AIR_IOR;
    float reflectance[3] = {1.0f, 1.0f, 1.0f}, transmittance[3] = {1.0f, 1.0f, 1.0f};
    parse_element(rd, [&](const std::string& name, const std::vector<Attr>& attrs, int&, int64_t&) {
        if (name == "rgb") {
            float c[3];
            const std::string* n = try_find_attr(attrs, "name");
            // `if let Ok(v) = parse_rgb(.., "specular_reflectance") .. else if let Ok(v) = parse_rgb(.., "specular_transmittance")`:
            // a bad NUMBER under the right name panics in the reference; a missing value falls through to the last branch
            if (n && *n == "specular_reflectance" && try_find_attr(attrs, "value")) {
                parse_rgb(attrs, "specular_reflectance", c);
                std::memcpy(reflectance, c, sizeof(c));
            } else if (n && *n == "specular_transmittance" && try_find_attr(attrs, "value")) {
                parse_rgb(attrs, "specular_transmittance", c);
                std::memcpy(transmittance, c, sizeof(c));
            } else {
                fail("Unknown dielectric rgb data '" + find_attr(attrs, "name") + "'");
            }
        } else if (name == "float") {
            const std::string& n = find_attr(attrs, "name");
            const float v = parse_f32(find_attr(attrs, "value"), "float " + n);
            if (n == "int_ior") int_ior = v;
            else if (n == "ext_ior") ext_ior = v;
            else fail("Unknown dielectric float data '" + n + "'");
        } else {
            fail("Unknown dielectric data type '" + name + "'");
        }
    });
    // abs_diff_eq!(ext_ior, AIR_IOR, epsilon = 0.001)
    const float diff = ext_ior > AIR_IOR ? ext_ior - AIR_IOR : AIR_IOR - ext_ior;
    if (!(diff <= EXT_IOR_EPSILON)) {
        char buf[64];
        for (int digits = 1; digits <= 9; ++digits) {  // the shortest decimal that reads back, as Rust's `{}` prints an f32
            std::snprintf(buf, sizeof(buf), "%.*g", digits, (double)ext_ior);
            if (std::strtof(buf, nullptr) == ext_ior) break;
        }
        fail(std::string("Only air supported for external IoR not supported but received '") + buf + "'");
    }
    return make_mat(YK_MAT_GLASS, reflectance, transmittance, int_ior, false);
}

// emitter.rs:43-65
void parse_constant_emitter(XmlReader& rd, float radiance[3]) {
    radiance[0] = radiance[1] = radiance[2] = 0.0f;
    parse_element(rd, [&](const std::string& name, const std::vector<Attr>& attrs, int&, int64_t&) {
        if (name == "rgb") parse_rgb(attrs, "radiance", radiance);
        else fail("Unknown constant emitter data type '" + name + "'");
    });
}
// emitter.rs:67-115
yk_light_desc parse_point_light(XmlReader& rd) {
    float position[3] = {0.0f, 0.0f, 0.0f}, intensity[3] = {0.0f, 0.0f, 0.0f};
    parse_element(rd, [&](const std::string& name, const std::vector<Attr>& attrs, int&, int64_t&) {
        if (name == "point") {
            if (find_attr(attrs, "name") != "position") fail("Expected 'name': 'filename' as first mesh 'string' attribute");  // sic
            for (size_t i = 1; i < attrs.size(); ++i) {  // skip(1): `name` is assumed to come first
                const std::string& a = attrs[i].name;
                float* dst = a == "x" ? &position[0] : (a == "y" ? &position[1] : (a == "z" ? &position[2] : nullptr));
                if (!dst) fail("Invalid point axis '" + a + "'");
                *dst = parse_f32(attrs[i].value, "point");
            }
        } else if (name == "rgb") {
            parse_rgb(attrs, "intensity", intensity);
        } else {
            fail("Unknown light data type '" + name + "'");
        }
    });
    position[0] = -position[0];  // Mitsuba's +X is to the left of +Z
    Xf tr = xf_translation(position[0], position[1], position[2]);
    yk_light_desc l;
    yk_make_point_light(tr.m, intensity, &l);
    return l;
}
// emitter.rs:117-163
yk_light_desc parse_spot_light(XmlReader& rd) {
    Xf light_to_world = xf_identity();
    float intensity[3] = {0.0f, 0.0f, 0.0f}, total_width_degrees = 0.0f, falloff_start_degrees = 0.0f;
    parse_element(rd, [&](const std::string& name, const std::vector<Attr>& attrs, int& level, int64_t&) {
        if (name == "float") {
            const std::string& n = find_attr(attrs, "name");
            if (n == "cutoff_angle") total_width_degrees = parse_f32(find_attr(attrs, "value"), "float cutoff_angle");
            else if (n == "beam_width") falloff_start_degrees = parse_f32(find_attr(attrs, "value"), "float beam_width");
            else fail("Unexpected spot light float 'name': '" + n + "'");
        } else if (name == "transform") {
            light_to_world = parse_transform(rd);
            level -= 1;
        } else if (name == "rgb") {
            parse_rgb(attrs, "intensity", intensity);
        } else {
            fail("Unknown spot light data type '" + name + "'");
        }
    });
    light_to_world = xf_mul(xf_scale(-1.0f, 1.0f, 1.0f), light_to_world);
    yk_light_desc l;
    if (yk_make_spot_light(light_to_world.m, light_to_world.mi, intensity, total_width_degrees, falloff_start_degrees, &l) != YK_OK) fail("Invalid spot light");
    return l;
}

bool path_exists(const std::string& p) {
    struct stat sb;
    return ::stat(p.c_str(), &sb) == 0;
}

struct ShapeRec : PlyJob {
    Xf transform;
    int material = 0;
};

// shape::parse (shape.rs:19-94) up to the call of ply::load, which is recorded as a job
void parse_shape(XmlReader& rd, const std::string& dir, const std::map<std::string, int>& materials, const std::vector<Attr>& shape_attrs,
                 std::vector<std::unique_ptr<ShapeRec>>& shapes) {
    const std::string& type = find_attr(shape_attrs, "type");
    if (type != "ply") fail("Unexpected shape type '" + type + "'!");
    Xf transform = xf_identity();
    std::string ply_path, material_id;
    bool have_path = false, have_material = false;
    parse_element(rd, [&](const std::string& name, const std::vector<Attr>& attrs, int& level, int64_t&) {
        if (name == "string") {
            if (find_attr(attrs, "name") != "filename") fail("Expected 'name': 'filename' as mesh 'string' attribute");
            std::string rel = find_attr(attrs, "value");
            for (char& c : rel)
                if (c == '\\') c = '/';
            // Path::join: an absolute second path replaces the first; canonicalize(): the file must exist
            ply_path = (!rel.empty() && rel[0] == '/') ? rel : dir + "/" + rel;
            if (!path_exists(ply_path)) fail("Could not open '" + ply_path + "'");
            have_path = true;
        } else if (name == "ref") {
            const std::string& ref_type = find_attr(attrs, "name");
            if (ref_type != "bsdf") fail("Expected mesh 'ref' to be 'bsdf', got '" + ref_type + "'");
            material_id = find_attr(attrs, "id");
            have_material = true;
        } else if (name == "transform") {
            transform = parse_transform(rd);
            level -= 1;
        } else {
            fail("Unknown shape type '" + name + "'");
        }
    });
    transform = xf_mul(xf_scale(-1.0f, 1.0f, 1.0f), transform);
    if (!have_path) fail("Mesh with no ply");
    if (!have_material) fail("Mesh with no material");
    auto it = materials.find(material_id);
    if (it == materials.end()) fail("Unknown mesh material '" + material_id + "'");
    std::unique_ptr<ShapeRec> rec(new ShapeRec());
    rec->ply_path = ply_path;
    rec->transform = transform;
    rec->material = it->second;
    shapes.push_back(std::move(rec));
}

// mitsuba::load, mod.rs:28-218
yk_status load_mitsuba(const std::string& path, yk_loaded_scene& s) {
    std::vector<unsigned char> bytes;
    if (!read_file(path, bytes)) return lfail(YK_ERR_INVALID_ARGUMENT, "Could not open '" + path + "'");
    XmlReader rd;
    rd.in.assign(bytes.begin(), bytes.end());
    if (rd.in.compare(0, 3, "\xEF\xBB\xBF") == 0) rd.in.erase(0, 3);
    std::string dir = ".";
    {
        size_t slash = path.find_last_of('/');
        if (slash != std::string::npos) dir = slash == 0 ? "/" : path.substr(0, slash);
    }
    std::map<std::string, int> materials;
    std::vector<std::unique_ptr<ShapeRec>> shapes;
    yk_status st = YK_OK;
    std::string error;
    try {
        int64_t ignore_level = -1;
        for (bool more = true; more;) {
            Ev e = rd.next();
            switch (e.kind) {
                case Ev::Start: {
                    if (ignore_level < 0) {
                        const std::string& name = e.name;
                        if (name == "scene") {
                            if (find_attr(e.attrs, "version") != "2.1.0") fail("Scene file version is not 2.1.0");
                        } else if (name == "default") {
                            const std::string& n = find_attr(e.attrs, "name");
                            const std::string& v = find_attr(e.attrs, "value");
                            if (n == "resx") s.camera.res_x = parse_u16(v, "default resx");
                            else if (n == "resy") s.camera.res_y = parse_u16(v, "default resy");
                        } else if (name == "integrator") {
                            ignore_level = 0;
                        } else if (name == "sensor") {
                            parse_sensor(rd, s.camera);
                        } else if (name == "bsdf") {
                            const std::string& type = find_attr(e.attrs, "type");
                            yk_material_desc m;
                            if (type == "twosided") m = parse_twosided(rd);
                            else if (type == "diffuse") m = parse_diffuse(rd);
                            else if (type == "dielectric") m = parse_dielectric(rd);
                            else fail("Unknown bsdf type '" + type + "'");
                            const std::string& id = find_attr(e.attrs, "id");
                            s.materials.push_back(m);
                            materials[id] = (int)s.materials.size() - 1;  // HashMap::insert replaces
                        } else if (name == "emitter") {
                            const std::string& type = find_attr(e.attrs, "type");
                            if (type == "constant") parse_constant_emitter(rd, s.background);
                            else if (type == "point") s.lights.push_back(parse_point_light(rd));
                            else if (type == "spot") s.lights.push_back(parse_spot_light(rd));
                            else ignore_level = 0;
                        } else if (name == "shape") {
                            parse_shape(rd, dir, materials, e.attrs, shapes);
                        } else {
                            fail("Unknown element: '" + name + "'");
                        }
                    }
                    if (ignore_level >= 0) ignore_level += 1;
                    break;
                }
                case Ev::End:
                    if (ignore_level >= 0) {
                        const int64_t level_after = ignore_level - 1;
                        ignore_level = level_after > 0 ? level_after : -1;
                    }
                    break;
                case Ev::PI: fail("Unexpected processing instruction: " + e.name);
                case Ev::CData: fail("Unexpected CDATA: " + e.name);
                case Ev::Chars: fail("Unexpected characters outside tags: " + e.name);
                case Ev::Doctype: fail("DOCTYPE declarations are not supported", YK_ERR_UNSUPPORTED);
                case Ev::Space: break;
                case Ev::EndDoc:
                case Ev::Error: more = false; break;  // "XML error": the scene is built from what was read
            }
        }
    } catch (const Fail& f) {
        st = f.st;
        error = f.msg + " (" + path + ")";
    }
    // The reference loads each PLY inside shape::parse, so the first failure in DOCUMENT order wins: a PLY of a shape that was
    // complete before the parse stopped comes before the parse error.  The files are read here, by the pool.
    std::vector<PlyJob*> jobs;
    for (auto& sh : shapes) jobs.push_back(sh.get());
    read_ply_jobs(jobs, true);
    for (auto& sh : shapes)
        if (sh->status != YK_OK) return lfail(sh->status, sh->error);
    if (st != YK_OK) return lfail(st, error);
    if (shapes.empty()) return lfail(YK_ERR_INVALID_ARGUMENT, "mitsuba: scene has no shapes (" + path + ")");
    size_t nv = 0, nt = 0;
    for (auto& sh : shapes) {
        nv += sh->ply.pts.size() / 3;
        nt += sh->ply.indices.size() / 3;
    }
    s.points.reserve(3 * nv);
    s.normals.reserve(3 * nv);
    s.uvs.reserve(2 * nv);
    s.indices.reserve(3 * nt);
    s.tri_mesh.reserve(nt);
    s.tri_material.reserve(nt);
    s.tri_area_light.reserve(nt);
    s.shape_order.reserve(nt);
    // "default target to middle way into the visible scene" (mod.rs:192-203): the BVH's root box is the union of the shapes'
    // bounds, i.e. of the vertices that belong to a triangle — a mesh's whole vertex range where the file has no stray vertex
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    auto grow = [&](size_t vertex) {
        for (int k = 0; k < 3; ++k) {
            lo[k] = rmin(lo[k], s.points[3 * vertex + k]);
            hi[k] = rmax(hi[k], s.points[3 * vertex + k]);
        }
    };
    for (auto& sh : shapes) {
        const size_t v0 = s.points.size() / 3, i0 = s.indices.size();
        add_ply_mesh(s, sh->ply, &sh->transform, sh->material);
        if (sh->all_referenced)
            for (size_t v = v0; v < s.points.size() / 3; ++v) grow(v);
        else
            for (size_t i = i0; i < s.indices.size(); ++i) grow(s.indices[i]);
        PlyMesh().pts.swap(sh->ply.pts);
    }
    s.shape_order_flat = s.shape_order;
    yk_camera_params& c = s.camera;
    const V3 position{c.position[0], c.position[1], c.position[2]};
    const V3 fwd = normalize(V3{c.target[0], c.target[1], c.target[2]} - position);
    // Bounds3::intersections / slab_test (math/bounds.rs:176-206) with t_max = inf
    const V3 inv{1.0f / fwd.x, 1.0f / fwd.y, 1.0f / fwd.z};
    const V3 t0{(lo[0] - position.x) * inv.x, (lo[1] - position.y) * inv.y, (lo[2] - position.z) * inv.z};
    const V3 t1{(hi[0] - position.x) * inv.x, (hi[1] - position.y) * inv.y, (hi[2] - position.z) * inv.z};
    const float p0 = rmax(rmax(rmax(rmin(t0.x, t1.x), rmin(t0.y, t1.y)), rmin(t0.z, t1.z)), 0.0f);
    const float p1 = rmin(rmin(rmin(rmax(t0.x, t1.x), rmax(t0.y, t1.y)), rmax(t0.z, t1.z)), INFINITY);
    if (p0 <= p1) {
        const V3 target = p0 > 0.0f ? position + fwd * ((p0 + p1) / 2.0f) : position + fwd * (p1 / 2.0f);
        c.target[0] = target.x; c.target[1] = target.y; c.target[2] = target.z;
    }
    return YK_OK;
}

}  // namespace

extern "C" {

yk_status yk_load_mitsuba(const char* path, uint32_t split_method, uint32_t max_shapes_in_node, yk_loaded_scene** out) {
    if (!path || !out) return lfail(YK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    yk_status st;
    yk_loaded_scene* s = nullptr;
    try {
        s = new yk_loaded_scene();
        default_camera(*s);
        s->split_method = split_method;
        s->max_shapes_in_node = max_shapes_in_node;
        st = load_mitsuba(path, *s);
    } catch (const std::exception& e) {  // e.g. bad_alloc on an absurd element count
        st = lfail(YK_ERR_INVALID_ARGUMENT, std::string("mitsuba: ") + e.what());
    }
    if (st != YK_OK) {
        delete s;
        return st;
    }
    *out = s;
    return YK_OK;
}

yk_status yk_load_scene(const char* path, uint32_t split_method, uint32_t max_shapes_in_node, yk_loaded_scene** out) {
    if (!path || !out) return lfail(YK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    try {
        const std::string p(path);
        if (p.empty()) return lfail(YK_ERR_INVALID_ARGUMENT, "Empty path: the built-in scene is constructed by the caller");
        if (!path_exists(p)) return lfail(YK_ERR_INVALID_ARGUMENT, "Scene does not exist '" + p + "'");
        // Path::extension: of the last component, after its last '.', none for "name" and ".name"
        size_t end = p.size();
        while (end > 1 && p[end - 1] == '/') --end;
        size_t slash = p.find_last_of('/', end - 1);
        const std::string file = p.substr(slash == std::string::npos ? 0 : slash + 1, end - (slash == std::string::npos ? 0 : slash + 1));
        size_t dot = file.find_last_of('.');
        if (dot == std::string::npos || dot == 0 || file == "..") return lfail(YK_ERR_INVALID_ARGUMENT, "Expected a file with an extension");
        const std::string ext = file.substr(dot + 1);
        if (ext == "ply") return yk_load_ply(path, split_method, max_shapes_in_node, out);
        if (ext == "xml") return yk_load_mitsuba(path, split_method, max_shapes_in_node, out);
        if (ext == "pbrt") return yk_load_pbrt(path, split_method, max_shapes_in_node, out);
        return lfail(YK_ERR_INVALID_ARGUMENT, "Unknown extension '" + ext + "'");
    } catch (const std::exception& e) {
        return lfail(YK_ERR_INVALID_ARGUMENT, std::string("load: ") + e.what());
    }
}

}  // extern "C"
