// snn/color.h -- the colour formats the hot path uses (reference core/inc/snn/color.h:20-110).
#pragma once
#include <cstddef>
namespace snn {
// the 8-bit ones (reference names) and the 16-bit ones (10 / 12 / 16-bit video in 2-byte containers; appended): a model's input / output frame
enum class ColorFormat { NONE, RGBA32F, RGBA16F, R32F, R8, RGB8, RGBA8, R16, RGB16, RGBA16 };
inline bool isFrame16Format(ColorFormat f) { return f == ColorFormat::R16 || f == ColorFormat::RGB16 || f == ColorFormat::RGBA16; }
inline bool isFrameFormat(ColorFormat f) { return f == ColorFormat::R8 || f == ColorFormat::RGB8 || f == ColorFormat::RGBA8 || isFrame16Format(f); }
struct ColorFormatDesc {
    const char* name;
    size_t bits, ch;
    size_t bytes() const { return bits / 8U; }
};
inline ColorFormatDesc getColorFormatDesc(ColorFormat f) {
    switch (f) {
    case ColorFormat::RGBA32F: return {"RGBA32F", 128, 4};
    case ColorFormat::RGBA16F: return {"RGBA16F", 64, 4};
    case ColorFormat::R32F: return {"R32F", 32, 1};
    case ColorFormat::R8: return {"R8", 8, 1};
    case ColorFormat::RGB8: return {"RGB8", 24, 3};
    case ColorFormat::RGBA8: return {"RGBA8", 32, 4};
    case ColorFormat::R16: return {"R16", 16, 1};
    case ColorFormat::RGB16: return {"RGB16", 48, 3};
    case ColorFormat::RGBA16: return {"RGBA16", 64, 4};
    default: return {"NONE", 0, 0};
    }
}
} // namespace snn
