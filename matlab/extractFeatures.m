function [features, validPoints] = extractFeatures(I, points, varargin)
%EXTRACTFEATURES libvo (MI355X) shadow for extractFeatures(I, points, "Method", "SIFT").
%   [features, validPoints] = extractFeatures(I, points, "Method", "SIFT")
%   reference call site: VO.m:83-84.  Returns the N x 128 single descriptors
%   of these points of this image; every point gets a descriptor (validPoints = points).
%   For any subset or permutation of the detectSIFTFeatures shadow's last detections of
%   this image, e.g. selectStrongest(points, N), they are the descriptors that shadow
%   computed in the same device pass (vo_mex('strongest', N) selects on the device
%   instead).  Any other SIFTPoints -- moved, rescaled or re-oriented detections, points
%   of another detector, a grid, SIFTPoints(...) built by hand (Octave 0, Layer 0) -- are
%   described on the device by vo_mex('describe', ...): Location, Scale, Orientation,
%   Octave and Layer are read; libvo's rules for them are in include/vo.h.
    if numel(varargin) ~= 2 || ~strcmpi(string(varargin{1}), "Method") || ~strcmpi(string(varargin{2}), "SIFT")
        error('vo:extractFeatures:options', 'libvo implements extractFeatures(I, points, "Method", "SIFT") only');
    end
    if ~isa(I, 'uint8')
        I = im2uint8(I);
    end
    key = [points.Location, points.Scale, points.Orientation];
    desc = vo_sift_cache('get', I, key);
    if isempty(desc) && points.Count > 0   % not among the last detections of this image: detect again
        [loc, scale, ori, ~, all_desc] = vo_mex('sift', I);
        [found, row] = ismember(key, [loc, scale, ori], 'rows');
        if all(found)
            desc = all_desc(row, :);
        else
            % not (all) this library's detections -- moved, rescaled or re-oriented points,
            % another detector's, a grid, SIFTPoints built by hand: describe exactly these
            % points on the device (vo_describe).  The lookups stay first: they are exact for
            % the library's own detections, whose degree -> radian -> degree round trip is not.
            desc = vo_mex('describe', I, points.Location, points.Scale, points.Orientation, ...
                          int32(points.Octave), int32(points.Layer));
        end
    end
    features = desc;
    validPoints = points;
end
